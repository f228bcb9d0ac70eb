// pvcompose.hip -- libpvcompose.so (include/pvcompose.h): multi-object training frames composed from a
// bank of single-object frames, the draw of their placement, and the blur + noise finish.  One
// translation unit that includes no other csrc/ file, so the other seven libraries' sources do not
// rebuild it.
//
//   k_vis_init  visible[f][s] = 0
//   k_compose   a lane owns kPx = 8 consecutive output pixels of a row, a block kThreads lanes, the grid is
//               (blocks per frame) x b, flattened (pvaugment.hip's shape).  The frame's slots and erasers go
//               to LDS once, each with its shifted box clipped to the output frame; a lane walks the slots
//               from S - 1 down, skips a slot whose box misses its 8 pixels without touching the source,
//               and stops when its 8 pixels are decided.  Per-slot pixel counts: LDS adds, then global adds.
//   k_cparams   one thread per frame: shifts, erasers, ksel, amp
//   k_finish    a block takes a kTile x kTile tile of one frame: the tile with its halo as u8 to LDS, the
//               horizontal pass to LDS as f32, the vertical pass, the noise and the store from there; a
//               frame with ksel = 0 and amp = 0 is a plain copy
// Nothing waits on anything but the stream's order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pvcompose.h"

namespace {

constexpr int kThreads = PV_CMP_THREADS;
constexpr int kPx = PV_CMP_PIXELS;
constexpr int kTile = PV_CMP_TILE;
constexpr int kHalo = PV_CMP_HALO;
constexpr int kTileH = kTile + 2 * kHalo;
static_assert(kPx == 8, "the group stores below are written for 8 pixels");
static_assert(PV_CMP_MAX_SLOTS <= 32 && PV_CMP_MAX_ERASE <= 32, "lanes 0..31 fill the slot table, 32..63 the erasers");

inline int rc(hipError_t e) { return e == hipSuccess ? PV_OK : (int)e; }
inline int last() { return rc(hipGetLastError()); }

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
constexpr uint64_t G = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ int64_t load_label(const void *base, int kind, int64_t off) {
    if (kind == PV_CMP_LABEL_U8) return (int64_t)((const uint8_t *)base)[off];
    if (kind == PV_CMP_LABEL_I32) return (int64_t)((const int32_t *)base)[off];
    return ((const int64_t *)base)[off];
}

// ---- pv_compose_apply --------------------------------------------------------------------------------------
struct ComposeArgs {
    pv_cmp_desc d;
    int32_t nblk;        // blocks per frame
    int32_t gw;          // groups of kPx pixels per output row
};

// One slot of the block's frame, ready for the lanes: the box is the shifted box clipped to the output
// frame, so x - dx and y - dy of a pixel inside it lie in the source's clipped box.
struct Slot {
    int64_t ibase, lbase;    // the source frame's first element in the bank's image and label map
    int64_t src_label;
    int32_t live;
    int32_t ox0, oy0, ox1, oy1;
    int32_t dx, dy;
    int32_t cls;
};

__global__ void k_vis_init(int32_t *visible, int32_t n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) visible[i] = 0;
}

__device__ __forceinline__ void store_ints(void *base, int kind, int64_t off, int64_t sx, int n, const int32_t (&v)[kPx]) {
    if (kind == PV_CMP_LABEL_U8) {
        uint8_t *p = (uint8_t *)base + off;
        if (sx == 1 && n == kPx && ((uintptr_t)p & 7) == 0) {
            uint2 w = make_uint2(0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                w.x |= ((uint32_t)v[e] & 255u) << (8 * e);
                w.y |= ((uint32_t)v[e + 4] & 255u) << (8 * e);
            }
            *(uint2 *)p = w;
        } else {
#pragma unroll
            for (int e = 0; e < kPx; ++e)
                if (e < n) p[e * sx] = (uint8_t)v[e];
        }
    } else if (kind == PV_CMP_LABEL_I32) {
        int32_t *p = (int32_t *)base + off;
#pragma unroll
        for (int e = 0; e < kPx; ++e)
            if (e < n) p[e * sx] = v[e];
    } else {
        int64_t *p = (int64_t *)base + off;
#pragma unroll
        for (int e = 0; e < kPx; ++e)
            if (e < n) p[e * sx] = (int64_t)v[e];
    }
}

__global__ __launch_bounds__(kThreads) void k_compose(ComposeArgs a) {
    __shared__ Slot s_slot[PV_CMP_MAX_SLOTS];
    __shared__ int32_t s_er[PV_CMP_MAX_ERASE][4];
    __shared__ int32_t s_vis[PV_CMP_MAX_SLOTS];
    const pv_cmp_desc &d = a.d;
    const int f = (int)(blockIdx.x / (uint32_t)a.nblk);
    const uint32_t blk = blockIdx.x - (uint32_t)f * (uint32_t)a.nblk;
    const int t = threadIdx.x;

    // the tables: every range check here, in 64-bit integers, before any address of the bank is formed
    if (t < d.S) {
        const int32_t *p = d.pick + ((int64_t)f * d.S + t) * 8;
        const int32_t *sh = d.shift + ((int64_t)f * d.S + t) * 2;
        const int32_t src = p[0], cls = p[2];
        const int32_t x0 = max(p[3], 0), y0 = max(p[4], 0), x1 = min(p[5], d.W - 1), y1 = min(p[6], d.H - 1);
        const int64_t dx = sh[0], dy = sh[1];
        const int64_t ox0 = max((int64_t)x0 + dx, (int64_t)0), ox1 = min((int64_t)x1 + dx, (int64_t)d.Wo - 1);
        const int64_t oy0 = max((int64_t)y0 + dy, (int64_t)0), oy1 = min((int64_t)y1 + dy, (int64_t)d.Ho - 1);
        const bool live = src >= 0 && src < d.N && cls >= 1 && cls <= d.ncls && x0 <= x1 && y0 <= y1 &&
                          ox0 <= ox1 && oy0 <= oy1;
        Slot q;
        q.live = live;
        q.ibase = live ? (int64_t)src * d.image_strides[0] : 0;
        q.lbase = live ? (int64_t)src * d.label_strides[0] : 0;
        q.src_label = p[1];
        q.ox0 = live ? (int32_t)ox0 : 0; q.ox1 = live ? (int32_t)ox1 : -1;
        q.oy0 = live ? (int32_t)oy0 : 0; q.oy1 = live ? (int32_t)oy1 : -1;
        q.dx = sh[0]; q.dy = sh[1];
        q.cls = cls;
        s_slot[t] = q;
        s_vis[t] = 0;
    }
    if (t >= 32 && t < 32 + d.E) {
        const int e = t - 32;
        const int32_t *p = d.erase + ((int64_t)f * d.E + e) * 4;
        s_er[e][0] = max(p[0], 0); s_er[e][1] = max(p[1], 0);
        s_er[e][2] = min(p[2], d.Wo - 1); s_er[e][3] = min(p[3], d.Ho - 1);
    }
    __syncthreads();

    const int64_t tt = (int64_t)blk * kThreads + t;
    const int y = (int)(tt / a.gw);
    const int x = (int)(tt - (int64_t)y * a.gw) * kPx;
    const int n = y < d.Ho ? min(kPx, d.Wo - x) : 0;

    int32_t inst[kPx], lab[kPx];
    uint8_t col[kPx][3];
#pragma unroll
    for (int e = 0; e < kPx; ++e) { inst[e] = 0; lab[e] = 0; col[e][0] = col[e][1] = col[e][2] = 0; }
    const int32_t is1 = (int32_t)d.image_strides[1], is2 = (int32_t)d.image_strides[2], is3 = (int32_t)d.image_strides[3];
    const int32_t ls1 = (int32_t)d.label_strides[1], ls2 = (int32_t)d.label_strides[2];
    int open = n;      // pixels of this lane no slot has taken yet
    for (int s = d.S - 1; s >= 0 && open > 0; --s) {
        const Slot &q = s_slot[s];
        if (!q.live || y < q.oy0 || y > q.oy1 || x + n - 1 < q.ox0 || x > q.ox1) continue;
        const int32_t sy = (int32_t)((int64_t)y - q.dy);
        const uint8_t *img = (const uint8_t *)d.image + q.ibase + sy * is1;
        const int32_t lrow = sy * ls1;
#pragma unroll
        for (int e = 0; e < kPx; ++e) {
            const int xe = x + e;
            if (e < n && inst[e] == 0 && xe >= q.ox0 && xe <= q.ox1) {      // inside the box: never past a row's box
                const int32_t sx = (int32_t)((int64_t)xe - q.dx);
                if (load_label(d.label, d.label_kind, q.lbase + lrow + sx * ls2) == q.src_label) {
                    inst[e] = s + 1;
                    lab[e] = q.cls;
                    const uint8_t *px = img + sx * is2;
                    col[e][0] = px[0]; col[e][1] = px[is3]; col[e][2] = px[2 * is3];
                    --open;
                }
            }
        }
    }

    // background or fill, then the erasers
    const uint8_t fill[3] = {(uint8_t)d.fill[0], (uint8_t)d.fill[1], (uint8_t)d.fill[2]};
    const uint8_t *bg_row = nullptr;
    if (d.background && n)
        bg_row = (const uint8_t *)d.background + (int64_t)f * d.background_strides[0] + (int64_t)y * d.background_strides[1];
    const int32_t bs2 = (int32_t)d.background_strides[2], bs3 = (int32_t)d.background_strides[3];
#pragma unroll
    for (int e = 0; e < kPx; ++e) {
        if (e >= n) continue;
        const int xe = x + e;
        bool erased = false;
        for (int k = 0; k < d.E; ++k)
            erased = erased || (xe >= s_er[k][0] && xe <= s_er[k][2] && y >= s_er[k][1] && y <= s_er[k][3]);
        if (erased) {
            inst[e] = 0; lab[e] = 0;
            col[e][0] = fill[0]; col[e][1] = fill[1]; col[e][2] = fill[2];
        } else if (inst[e] == 0) {
            if (bg_row) {
                const uint8_t *px = bg_row + xe * bs2;
                col[e][0] = px[0]; col[e][1] = px[bs3]; col[e][2] = px[2 * bs3];
            } else {
                col[e][0] = fill[0]; col[e][1] = fill[1]; col[e][2] = fill[2];
            }
        }
        if (inst[e] > 0) atomicAdd(&s_vis[inst[e] - 1], 1);
    }

    if (n) {
        const int64_t *s = d.out_image_strides;
        uint8_t *po = (uint8_t *)d.out_image + (int64_t)f * s[0] + (int64_t)y * s[1] + (int64_t)x * s[2];
        if (s[2] == 3 && s[3] == 1 && n == kPx && ((uintptr_t)po & 7) == 0) {
            uint32_t w[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int e = 0; e < kPx; ++e)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int byte = e * 3 + ch;
                    w[byte >> 2] |= (uint32_t)col[e][ch] << (8 * (byte & 3));
                }
            ((uint2 *)po)[0] = make_uint2(w[0], w[1]);
            ((uint2 *)po)[1] = make_uint2(w[2], w[3]);
            ((uint2 *)po)[2] = make_uint2(w[4], w[5]);
        } else {
#pragma unroll
            for (int e = 0; e < kPx; ++e)
                if (e < n) {
                    po[e * s[2]] = col[e][0]; po[e * s[2] + s[3]] = col[e][1]; po[e * s[2] + 2 * s[3]] = col[e][2];
                }
        }
        const int64_t *l = d.out_label_strides;
        store_ints(d.out_label, d.label_kind, (int64_t)f * l[0] + (int64_t)y * l[1] + (int64_t)x * l[2], l[2], n, lab);
        if (d.out_instance) {
            const int64_t *q = d.out_instance_strides;
            store_ints(d.out_instance, d.label_kind, (int64_t)f * q[0] + (int64_t)y * q[1] + (int64_t)x * q[2], q[2], n, inst);
        }
    }
    __syncthreads();
    if (t < d.S && s_vis[t] > 0) atomicAdd(&d.visible[(int64_t)f * d.S + t], s_vis[t]);
}

// ---- pv_compose_params -------------------------------------------------------------------------------------
struct ParamArgs {
    pv_cmp_ranges r;
    const int32_t *pick;
    const uint64_t *state;
    int32_t *shift, *erase, *ksel;
    float *amp;
};

__device__ __forceinline__ double draw(uint64_t base, int k) {
    return (double)(mix64(base + (uint64_t)(k + 1) * G) >> 11) * (1.0 / 9007199254740992.0);
}

// the clipped box and the shift of slot s; false (and a zero shift) for a slot that is dead or has an empty box
__device__ __forceinline__ bool place(const ParamArgs &a, int f, int s, uint64_t base, int32_t (&box)[4], int32_t &dx, int32_t &dy) {
    const pv_cmp_ranges &r = a.r;
    const int32_t *p = a.pick + ((int64_t)f * r.S + s) * 8;
    box[0] = max(p[3], 0); box[1] = max(p[4], 0); box[2] = min(p[5], r.W - 1); box[3] = min(p[6], r.H - 1);
    dx = 0; dy = 0;
    if (!(p[0] >= 0 && p[0] < r.N && p[2] >= 1 && p[2] <= r.ncls && box[0] <= box[2] && box[1] <= box[3])) return false;
    const double span = 1.0 - 2.0 * r.margin;
    const double tx = (r.margin + draw(base, PV_CMP_DRAW0 + 8 * s + 0) * span) * (double)(r.Wo - 1);
    const double ty = (r.margin + draw(base, PV_CMP_DRAW0 + 8 * s + 1) * span) * (double)(r.Ho - 1);
    dx = (int32_t)rint(tx - ((double)box[0] + (double)box[2]) / 2.0);
    dy = (int32_t)rint(ty - ((double)box[1] + (double)box[3]) / 2.0);
    return true;
}

__global__ void k_cparams(ParamArgs a) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const pv_cmp_ranges &r = a.r;
    if (f >= r.b) return;
    const uint64_t seed = a.state[0], n = a.state[1] + (uint64_t)f;
    const uint64_t base = mix64(mix64(seed + G) + (n + 1) * G);
    int32_t box[4], dx, dy;
    for (int s = 0; s < r.S; ++s) {
        place(a, f, s, base, box, dx, dy);
        int32_t *o = a.shift + ((int64_t)f * r.S + s) * 2;
        o[0] = dx; o[1] = dy;
    }
    for (int e = 0; e < r.E; ++e) {
        int32_t *o = a.erase + ((int64_t)f * r.E + e) * 4;
        if (!place(a, f, e % r.S, base, box, dx, dy)) {
            o[0] = 0; o[1] = 0; o[2] = -1; o[3] = -1;
            continue;
        }
        const int k = 192 + 8 * e;
        const int32_t bw = box[2] - box[0] + 1, bh = box[3] - box[1] + 1;
        const double fw = r.erase_frac[0] + draw(base, k + 0) * (r.erase_frac[1] - r.erase_frac[0]);
        const double fh = r.erase_frac[0] + draw(base, k + 1) * (r.erase_frac[1] - r.erase_frac[0]);
        const int32_t w = max(1, (int32_t)rint(fw * (double)bw)), h = max(1, (int32_t)rint(fh * (double)bh));
        const int32_t left = box[0] + dx + (int32_t)floor(draw(base, k + 2) * (double)(bw - w + 1));
        const int32_t top = box[1] + dy + (int32_t)floor(draw(base, k + 3) * (double)(bh - h + 1));
        o[0] = left; o[1] = top; o[2] = left + w - 1; o[3] = top + h - 1;
    }
    a.ksel[f] = draw(base, 256) < r.p_blur ? 1 + min(3, (int32_t)floor(4.0 * draw(base, 257))) : 0;
    a.amp[f] = (float)(r.noise[0] + draw(base, 258) * (r.noise[1] - r.noise[0]));
}

// ---- pv_compose_finish -------------------------------------------------------------------------------------
struct FinishArgs {
    pv_cmp_finish d;
    int32_t tx, ty;      // tiles per row and per column of a frame
};

// reflect-101 into 0..n - 1, for any i
__device__ __forceinline__ int reflect(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;      // inside: every pixel of an interior tile
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

__global__ __launch_bounds__(kThreads) void k_finish(FinishArgs a) {
    __shared__ uint8_t s_in[kTileH][kTileH][3];
    __shared__ float s_h[kTileH][kTile][3];
    const pv_cmp_finish &d = a.d;
    const uint32_t per = (uint32_t)a.tx * (uint32_t)a.ty;
    const int f = (int)(blockIdx.x / per);
    const uint32_t rem = blockIdx.x - (uint32_t)f * per;
    const int y0 = (int)(rem / (uint32_t)a.tx) * kTile, x0 = (int)(rem % (uint32_t)a.tx) * kTile;
    const int t = threadIdx.x;
    int j = d.ksel[f];
    if (j < 0 || j > 4) j = 0;
    const float amp = d.amp[f];
    const uint8_t *in = (const uint8_t *)d.image + (int64_t)f * d.image_strides[0];
    uint8_t *out = (uint8_t *)d.out + (int64_t)f * d.out_strides[0];
    const int32_t i1 = (int32_t)d.image_strides[1], i2 = (int32_t)d.image_strides[2], i3 = (int32_t)d.image_strides[3];
    const int32_t o1 = (int32_t)d.out_strides[1], o2 = (int32_t)d.out_strides[2], o3 = (int32_t)d.out_strides[3];

    if (j == 0 && amp == 0.0f) {     // uniform over the block: a plain copy
        for (int idx = t; idx < kTile * kTile * 3; idx += kThreads) {
            const int ch = idx % 3, lx = (idx / 3) % kTile, ly = idx / (3 * kTile);
            const int y = y0 + ly, x = x0 + lx;
            if (y < d.H && x < d.W) out[y * o1 + x * o2 + ch * o3] = in[y * i1 + x * i2 + ch * i3];
        }
        return;
    }

    for (int idx = t; idx < kTileH * kTileH * 3; idx += kThreads) {
        const int ch = idx % 3, rx = (idx / 3) % kTileH, ry = idx / (3 * kTileH);
        const int sy = reflect(y0 + ry - kHalo, d.H), sx = reflect(x0 + rx - kHalo, d.W);
        s_in[ry][rx][ch] = in[sy * i1 + sx * i2 + ch * i3];
    }
    __syncthreads();
    for (int idx = t; idx < kTileH * kTile * 3; idx += kThreads) {
        const int ch = idx % 3, lx = (idx / 3) % kTile, ry = idx / (3 * kTile);
        const uint8_t *v = &s_in[ry][lx + kHalo][ch];      // v[3 k]: the pixel k to the right
        float acc = (float)v[0];
        if (j > 0) {
            acc = d.w[j][0] * acc;
            for (int k = 1; k <= j; ++k) acc = acc + d.w[j][k] * ((float)v[-3 * k] + (float)v[3 * k]);
        }
        s_h[ry][lx][ch] = acc;
    }
    __syncthreads();
    const uint64_t key = mix64(mix64(d.state[0] + G) + (d.state[1] + (uint64_t)f + 1) * G);
    for (int idx = t; idx < kTile * kTile * 3; idx += kThreads) {
        const int ch = idx % 3, lx = (idx / 3) % kTile, ly = idx / (3 * kTile);
        const int y = y0 + ly, x = x0 + lx;
        if (y >= d.H || x >= d.W) continue;
        const float *h = &s_h[ly + kHalo][lx][ch];         // h[kTile * 3 * k]: the row k below
        float acc = h[0];
        if (j > 0) {
            acc = d.w[j][0] * acc;
            for (int k = 1; k <= j; ++k) acc = acc + d.w[j][k] * (h[-kTile * 3 * k] + h[kTile * 3 * k]);
        }
        const uint64_t p = (uint64_t)y * (uint64_t)d.W + (uint64_t)x;
        const uint64_t z = mix64(key + (((uint64_t)1 << 40) + 3 * p + (uint64_t)ch + 1) * G);
        const int32_t s = (int32_t)((z & 0xFFFF) + ((z >> 16) & 0xFFFF) + ((z >> 32) & 0xFFFF) + (z >> 48));
        const float tn = (float)(s - 131070) * (1.0f / 65536.0f);
        const float c = acc + amp * tn;
        out[y * o1 + x * o2 + ch * o3] = (uint8_t)(int)rintf(fminf(fmaxf(c, 0.0f), 255.0f));
    }
}

// ---- host ----------------------------------------------------------------------------------------------
bool dim_ok(int32_t v) { return v >= 1 && v <= PV_CMP_MAX_DIM; }
bool label_kind_ok(int32_t k) { return k == PV_CMP_LABEL_I64 || k == PV_CMP_LABEL_U8 || k == PV_CMP_LABEL_I32; }
uintptr_t label_mask(int32_t k) { return k == PV_CMP_LABEL_I64 ? 7 : k == PV_CMP_LABEL_I32 ? 3 : 0; }
bool is_finite(double v) { return v - v == 0.0; }

// a launch stays below 2^32 threads, which is what the runtime accepts: at most 2^24 - 1 blocks of kThreads lanes
constexpr int64_t kMaxBlocks = ((int64_t)1 << 32) / kThreads - 1;

int32_t groups_per_row(int32_t W) { return (W + kPx - 1) / kPx; }
// blocks per frame of k_compose; 0 if the flattened grid would exceed kMaxBlocks
int64_t compose_blocks(int32_t b, int32_t Ho, int32_t Wo) {
    const int64_t nblk = ((int64_t)Ho * groups_per_row(Wo) + kThreads - 1) / kThreads;
    return nblk * std::max<int64_t>(b, 1) <= kMaxBlocks ? nblk : 0;
}

// elements from the first to the last of an [n0][n1][n2] array with these strides (n2 == 1: two dimensions)
int64_t span(const int64_t *s, int64_t n0, int64_t n1, int64_t n2) {
    return (n0 - 1) * s[0] + (n1 - 1) * s[1] + (n2 > 1 ? (n2 - 1) * s[2] : 0);
}

bool counts_ok(int32_t N, int32_t S, int32_t E, int32_t ncls) {
    return N >= 1 && S >= 1 && S <= PV_CMP_MAX_SLOTS && E >= 0 && E <= PV_CMP_MAX_ERASE && ncls >= 1 && ncls <= PV_CMP_MAX_CLASSES;
}

}  // namespace

extern "C" {

int pv_compose_apply(const pv_cmp_desc *d, pv_stream_t stream) {
    if (!d) return PV_EINVAL;
    if (d->b < 0 || !dim_ok(d->H) || !dim_ok(d->W) || !dim_ok(d->Ho) || !dim_ok(d->Wo)) return PV_EINVAL;
    if (!counts_ok(d->N, d->S, d->E, d->ncls) || !label_kind_ok(d->label_kind)) return PV_EINVAL;
    if (d->label_kind == PV_CMP_LABEL_U8 && d->ncls > 255) return PV_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (d->image_strides[i] < 0 || d->background_strides[i] < 0 || d->out_image_strides[i] < 0) return PV_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (d->label_strides[i] < 0 || d->out_label_strides[i] < 0 || d->out_instance_strides[i] < 0) return PV_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (d->fill[i] < 0 || d->fill[i] > 255) return PV_EINVAL;
    // one frame of every operand spans at most 2^31 - 1 elements: the kernel's offsets inside one are 32-bit
    if (span(d->image_strides + 1, d->H, d->W, 3) > INT32_MAX || span(d->label_strides + 1, d->H, d->W, 1) > INT32_MAX ||
        span(d->out_image_strides + 1, d->Ho, d->Wo, 3) > INT32_MAX || span(d->out_label_strides + 1, d->Ho, d->Wo, 1) > INT32_MAX ||
        (d->out_instance && span(d->out_instance_strides + 1, d->Ho, d->Wo, 1) > INT32_MAX) ||
        (d->background && span(d->background_strides + 1, d->Ho, d->Wo, 3) > INT32_MAX))
        return PV_EINVAL;
    const int64_t nblk = compose_blocks(d->b, d->Ho, d->Wo);
    if (nblk == 0) return PV_EINVAL;
    if (d->b == 0) return PV_OK;
    if (!d->image || !d->label || !d->pick || !d->shift || !d->out_image || !d->out_label || !d->visible) return PV_EINVAL;
    if (d->E > 0 && !d->erase) return PV_EINVAL;
    const uintptr_t lm = label_mask(d->label_kind);
    if (((uintptr_t)d->label & lm) || ((uintptr_t)d->out_label & lm) || ((uintptr_t)d->out_instance & lm) ||
        (((uintptr_t)d->pick | (uintptr_t)d->shift | (uintptr_t)d->erase | (uintptr_t)d->visible) & 3))
        return PV_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int32_t nv = d->b * d->S;      // at most (2^24 - 1) * 16
    k_vis_init<<<dim3((unsigned)((nv + kThreads - 1) / kThreads)), kThreads, 0, st>>>(d->visible, nv);
    int e;
    if ((e = last())) return e;
    ComposeArgs a{*d, (int32_t)nblk, groups_per_row(d->Wo)};
    k_compose<<<dim3((unsigned)(nblk * d->b)), kThreads, 0, st>>>(a);
    return last();
}

int pv_compose_params(const pv_cmp_ranges *r, const int32_t *pick, const uint64_t *state, int32_t *shift, int32_t *erase,
                      int32_t *ksel, float *amp, pv_stream_t stream) {
    if (!r) return PV_EINVAL;
    if (r->b < 0 || !dim_ok(r->H) || !dim_ok(r->W) || !dim_ok(r->Ho) || !dim_ok(r->Wo)) return PV_EINVAL;
    if (!counts_ok(r->N, r->S, r->E, r->ncls)) return PV_EINVAL;
    if (!(r->margin >= 0.0) || !(r->margin <= 0.5)) return PV_EINVAL;
    if (!(r->erase_frac[0] > 0.0) || !(r->erase_frac[0] <= r->erase_frac[1]) || !(r->erase_frac[1] <= 1.0)) return PV_EINVAL;
    if (!(r->p_blur >= 0.0) || !(r->p_blur <= 1.0)) return PV_EINVAL;
    if (!is_finite(r->noise[0]) || !is_finite(r->noise[1]) || !(r->noise[0] >= 0.0) || !(r->noise[0] <= r->noise[1])) return PV_EINVAL;
    if (r->b == 0) return PV_OK;
    if (!pick || !state || !shift || !ksel || !amp || (r->E > 0 && !erase)) return PV_EINVAL;
    if (((uintptr_t)state & 7) ||
        (((uintptr_t)pick | (uintptr_t)shift | (uintptr_t)erase | (uintptr_t)ksel | (uintptr_t)amp) & 3))
        return PV_EALIGN;
    ParamArgs a{*r, pick, state, shift, erase, ksel, amp};
    k_cparams<<<dim3((unsigned)((r->b + 63) / 64)), 64, 0, (hipStream_t)stream>>>(a);
    return last();
}

int pv_compose_finish(const pv_cmp_finish *d, pv_stream_t stream) {
    if (!d) return PV_EINVAL;
    if (d->b < 0 || !dim_ok(d->H) || !dim_ok(d->W)) return PV_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (d->image_strides[i] < 0 || d->out_strides[i] < 0) return PV_EINVAL;
    for (int j = 0; j < 5; ++j)
        for (int t = 0; t <= j; ++t)
            if (!is_finite(d->w[j][t]) || !(d->w[j][t] >= 0.f)) return PV_EINVAL;
    if (span(d->image_strides + 1, d->H, d->W, 3) > INT32_MAX || span(d->out_strides + 1, d->H, d->W, 3) > INT32_MAX) return PV_EINVAL;
    const int32_t tx = (d->W + kTile - 1) / kTile, ty = (d->H + kTile - 1) / kTile;
    if ((int64_t)tx * ty * std::max<int64_t>(d->b, 1) > kMaxBlocks) return PV_EINVAL;
    if (d->b == 0) return PV_OK;
    if (!d->image || !d->out || !d->ksel || !d->amp || !d->state || d->image == d->out) return PV_EINVAL;
    if (((uintptr_t)d->state & 7) || (((uintptr_t)d->ksel | (uintptr_t)d->amp) & 3)) return PV_EALIGN;
    FinishArgs a{*d, tx, ty};
    k_finish<<<dim3((unsigned)((int64_t)tx * ty * d->b)), kThreads, 0, (hipStream_t)stream>>>(a);
    return last();
}

}  // extern "C"
