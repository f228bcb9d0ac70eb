// pvmodel.hip -- libpvmodel.so (include/pvmodel.h): bounding box, centroid, farthest-point keypoints
// and diameter of every model of a table.  One translation unit that includes no other csrc/ file,
// so the other four libraries' sources do not rebuild it.  Everything is fp64 with every operation
// rounded (-ffp-contract=off); no block ever waits on another block.
//
//   k_extent      one block of PV_MODEL_SUM_LANES threads per model: lane sums in the header's
//                 order, box and count through the same LDS tree
//   k_fps_block   one block of 1024 threads per model of at most PV_MODEL_BLOCK_MAX_PN points: the
//                 points in LDS, the running minimum in registers (12 per thread), all k steps inside
//   k_fps_step    the per-step form for larger models, one launch per step over (chunk, model):
//                 reduce the previous step's per-chunk partials to learn the last pick, update the
//                 chunk's running minimum in the workspace, write this chunk's partial; launch k
//                 only finishes pick k - 1
//   k_diam_pairs  (tile i, tile j >= i) x model: one point per thread in registers against the
//                 other tile in LDS; wave, then block, then one 64-bit integer atomicMax
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pvmodel.h"

namespace {

constexpr int kLanes = PV_MODEL_SUM_LANES;
constexpr int kBlockPn = PV_MODEL_BLOCK_MAX_PN;
constexpr int kFpsThreads = 1024;
constexpr int kFpsPer = kBlockPn / kFpsThreads;        // running minima per thread of k_fps_block
constexpr int kChunk = PV_MODEL_CHUNK;
constexpr int kStepThreads = 256;
constexpr int kStepPer = kChunk / kStepThreads;
constexpr int kTile = PV_MODEL_TILE;
constexpr int kNone = INT32_MAX;                       // index of "no candidate"
static_assert(kBlockPn % kFpsThreads == 0 && kChunk % kStepThreads == 0 && kTile % 64 == 0 && kLanes == 256, "tiling");

inline int rc(hipError_t e) { return e == hipSuccess ? PV_OK : (int)e; }
inline int last() { return rc(hipGetLastError()); }
inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

struct Partial {            // a chunk's (or a wave's) arg-max
    double v;
    int32_t i, pad;
};

struct Work {
    double *cen;            // [nmodels][3]
    int32_t *cnt;           // [nmodels]
    unsigned long long *acc;  // [nmodels]: 1 + the bits of the largest d2 so far, 0 = none
    double *md;             // [total]: the running minimum of the per-step form, by row of points
    Partial *part;          // [2][nmodels][chunks]
    size_t bytes;
};

inline int64_t chunks_of(int64_t n) { return std::max<int64_t>(1, (n + kChunk - 1) / kChunk); }

inline Work carve(void *base, int64_t nmodels, int64_t total) {
    Work w{};
    int64_t off = 0;
    char *p = (char *)base;
    w.cen = (double *)(p + off);              off = align_up(off + nmodels * 24, 256);
    w.cnt = (int32_t *)(p + off);             off = align_up(off + nmodels * 4, 256);
    w.acc = (unsigned long long *)(p + off);  off = align_up(off + nmodels * 8, 256);
    w.md = (double *)(p + off);               off = align_up(off + total * 8, 256);
    w.part = (Partial *)(p + off);            off = align_up(off + 2 * nmodels * chunks_of(total) * (int64_t)sizeof(Partial), 256);
    w.bytes = (size_t)off;
    return w;
}

// --------------------------------------------------------------------------
struct Range {
    int lo, n;
    bool ok;
};

__device__ inline Range model_range(const pv_model_points &p, int m) {
    const int lo = p.off[m], hi = p.off[m + 1];
    Range r;
    r.ok = lo >= 0 && hi >= lo && hi <= p.total && hi - lo <= p.max_pn;
    r.lo = lo;
    r.n = r.ok ? hi - lo : 0;
    return r;
}

// row of points, widened; false for an absent point (a non-finite coordinate)
__device__ inline bool load_point(const float *pts, int64_t row, double &x, double &y, double &z) {
    const float *q = pts + row * 3;
    const float fx = q[0], fy = q[1], fz = q[2];
    x = (double)fx;
    y = (double)fy;
    z = (double)fz;
    return isfinite(fx) && isfinite(fy) && isfinite(fz);
}

__device__ inline double d2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ inline double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

struct Best {
    double v;
    int i;
};

// the larger value, and of equal values the lower index: a total order, so any reduction shape
// gives the same winner
__device__ inline void take(Best &b, double v, int i) {
    if (v > b.v || (v == b.v && i < b.i)) {
        b.v = v;
        b.i = i;
    }
}

__device__ inline Best wave_best(Best b) {
    for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_xor(b.v, o);
        const int i = __shfl_xor(b.i, o);
        take(b, v, i);
    }
    return b;
}

// slot: WAVES entries of LDS nobody else touches until the caller's next barrier but one
template <int WAVES>
__device__ inline Best block_best(Best b, Partial *slot) {
    b = wave_best(b);
    if ((threadIdx.x & 63) == 0) {
        slot[threadIdx.x >> 6].v = b.v;
        slot[threadIdx.x >> 6].i = b.i;
    }
    __syncthreads();
    Best r{-1.0, kNone};
    for (int w = 0; w < WAVES; ++w) take(r, slot[w].v, slot[w].i);
    return r;
}

// --------------------------------------------------------------------------
__global__ __launch_bounds__(kLanes) void k_extent(pv_model_points p, double *bbox, double *cen, int32_t *cnt) {
    __shared__ double s_sum[3][kLanes], s_min[3][kLanes], s_max[3][kLanes];
    __shared__ int32_t s_cnt[kLanes];
    const int m = blockIdx.x, t = threadIdx.x;
    const Range r = model_range(p, m);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double sum[3] = {0.0, 0.0, 0.0}, mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    int c = 0;
    for (int i = t; i < r.n; i += kLanes) {
        double q[3];
        if (!load_point(p.points, (int64_t)r.lo + i, q[0], q[1], q[2])) continue;
        ++c;
        for (int e = 0; e < 3; ++e) {
            sum[e] += q[e];
            const double z = q[e] + 0.0;                 // a zero bound is +0.0 whatever the order
            mn[e] = z < mn[e] ? z : mn[e];
            mx[e] = z > mx[e] ? z : mx[e];
        }
    }
    for (int e = 0; e < 3; ++e) {
        s_sum[e][t] = sum[e];
        s_min[e][t] = mn[e];
        s_max[e][t] = mx[e];
    }
    s_cnt[t] = c;
    __syncthreads();
    for (int s = kLanes / 2; s > 0; s >>= 1) {
        if (t < s) {
            for (int e = 0; e < 3; ++e) {
                s_sum[e][t] += s_sum[e][t + s];
                s_min[e][t] = s_min[e][t + s] < s_min[e][t] ? s_min[e][t + s] : s_min[e][t];
                s_max[e][t] = s_max[e][t + s] > s_max[e][t] ? s_max[e][t + s] : s_max[e][t];
            }
            s_cnt[t] += s_cnt[t + s];
        }
        __syncthreads();
    }
    if (t < 3) {
        const int n = s_cnt[0];
        if (cen) cen[m * 3 + t] = n > 0 ? s_sum[t][0] / (double)n : qnan();
        if (bbox) {
            bbox[m * 6 + t] = n > 0 ? s_min[t][0] : qnan();
            bbox[m * 6 + 3 + t] = n > 0 ? s_max[t][0] : qnan();
        }
        if (cnt && t == 0) cnt[m] = n;
    }
}

// --------------------------------------------------------------------------
struct FpsArgs {
    pv_model_points p;
    int32_t k, start;
    const int32_t *start_idx;
    int32_t *idx;
    double *picked, *pick_d2;
    Work w;
    int32_t cpm;            // chunks per model of the per-step form's grid
    int32_t step;
};

__device__ inline void write_pick(const FpsArgs &a, int m, int j, int i, double v, double x, double y, double z) {
    const int64_t o = (int64_t)m * a.k + j;
    a.idx[o] = i;
    if (a.pick_d2) a.pick_d2[o] = v;
    if (a.picked) {
        a.picked[o * 3 + 0] = x;
        a.picked[o * 3 + 1] = y;
        a.picked[o * 3 + 2] = z;
    }
}

__device__ inline void write_dead(const FpsArgs &a, int m, int j) {
    write_pick(a, m, j, -1, qnan(), qnan(), qnan(), qnan());
}

__global__ __launch_bounds__(kFpsThreads) void k_fps_block(FpsArgs a) {
    extern __shared__ double smem[];
    Partial *slot = (Partial *)smem;                       // [2][16]
    float *pts = (float *)(smem + 2 * (kFpsThreads / 64) * (sizeof(Partial) / sizeof(double)));
    const int m = blockIdx.x, t = threadIdx.x;
    const Range r = model_range(a.p, m);
    if (r.ok && r.n > kBlockPn) return;                    // the per-step form's
    const int n = r.n;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    // everything that decides `dead` is the same in every thread of the block
    bool dead = !r.ok || n == 0;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    int s0 = -1;
    if (!dead) {
        if (a.start == PV_FPS_START_INDEX) {
            s0 = a.start_idx[m];
            double x, y, z;
            dead = s0 < 0 || s0 >= n || !load_point(a.p.points, (int64_t)r.lo + s0, x, y, z);
        } else if (a.w.cnt[m] == 0) {
            dead = true;
        } else {
            cx = a.w.cen[m * 3 + 0];
            cy = a.w.cen[m * 3 + 1];
            cz = a.w.cen[m * 3 + 2];
        }
    }
    if (dead) {
        for (int j = t; j < a.k; j += kFpsThreads) write_dead(a, m, j);
        return;
    }
    // the points into LDS; md: the running minimum of point t + e * 1024, negative = absent
    double md[kFpsPer];
    Best b{-1.0, kNone};
#pragma unroll
    for (int e = 0; e < kFpsPer; ++e) {
        const int i = t + e * kFpsThreads;
        md[e] = -1.0;
        if (i < n) {
            const float *q = a.p.points + ((int64_t)r.lo + i) * 3;
            const float fx = q[0], fy = q[1], fz = q[2];
            pts[3 * i + 0] = fx;
            pts[3 * i + 1] = fy;
            pts[3 * i + 2] = fz;
            if (isfinite(fx) && isfinite(fy) && isfinite(fz)) {
                if (a.start == PV_FPS_START_INDEX) {
                    md[e] = inf;
                } else {
                    md[e] = d2((double)fx, (double)fy, (double)fz, cx, cy, cz);
                    take(b, md[e], i);
                }
            }
        }
    }
    Best pick{inf, s0};
    if (a.start != PV_FPS_START_INDEX) {
        pick = block_best<kFpsThreads / 64>(b, slot);       // its barrier also publishes pts
        if (a.start == PV_FPS_START_CENTROID) {
#pragma unroll
            for (int e = 0; e < kFpsPer; ++e) md[e] = md[e] < 0.0 ? -1.0 : inf;
        }
    } else {
        __syncthreads();
    }
    if (pick.i < 0 || pick.i >= n) {                        // cannot happen with count > 0; never index LDS with it
        for (int j = t; j < a.k; j += kFpsThreads) write_dead(a, m, j);
        return;
    }
    for (int j = 0; j < a.k; ++j) {
        const double px = (double)pts[3 * pick.i + 0], py = (double)pts[3 * pick.i + 1], pz = (double)pts[3 * pick.i + 2];
        if (t == 0) write_pick(a, m, j, pick.i, pick.v, px, py, pz);
        if (j + 1 == a.k) break;
        b = Best{-1.0, kNone};
#pragma unroll
        for (int e = 0; e < kFpsPer; ++e) {
            const int i = t + e * kFpsThreads;
            if (md[e] >= 0.0) {
                const double d = d2((double)pts[3 * i + 0], (double)pts[3 * i + 1], (double)pts[3 * i + 2], px, py, pz);
                md[e] = d < md[e] ? d : md[e];
                take(b, md[e], i);
            }
        }
        // the two slot rows alternate: a row is rewritten only after a barrier every reader of it has passed
        pick = block_best<kFpsThreads / 64>(b, slot + ((j + 1) & 1) * (kFpsThreads / 64));
    }
}

__global__ __launch_bounds__(kStepThreads) void k_fps_step(FpsArgs a) {
    __shared__ Partial slot[2][kStepThreads / 64];
    const int m = blockIdx.y, c = blockIdx.x, t = threadIdx.x, j = a.step;
    const Range r = model_range(a.p, m);
    if (!r.ok || r.n <= kBlockPn) return;                  // skipped (k_fps_block reports it), or k_fps_block's
    const int n = r.n, nch = (n + kChunk - 1) / kChunk;
    if (c >= nch) return;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    Partial *prev = a.w.part + ((int64_t)((j + 1) & 1) * a.p.nmodels + m) * a.cpm;
    Partial *cur = a.w.part + ((int64_t)(j & 1) * a.p.nmodels + m) * a.cpm;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (j > 0) {
        // the last pick: every block of the model reduces the same partials and gets the same answer
        Best b{-1.0, kNone};
        for (int q = t; q < nch; q += kStepThreads) take(b, prev[q].v, prev[q].i);
        const Best pick = block_best<kStepThreads / 64>(b, slot[0]);
        const bool dead = pick.i < 0 || pick.i >= n;       // kNone, or nothing this kernel wrote
        if (!dead) load_point(a.p.points, (int64_t)r.lo + pick.i, px, py, pz);
        if (c == 0 && t == 0) {
            if (dead) write_dead(a, m, j - 1);
            else write_pick(a, m, j - 1, pick.i, pick.v, px, py, pz);
        }
        if (j == a.k) return;                              // the finishing launch
        if (dead) {                                        // and stays dead
            if (t == 0) {
                cur[c].v = -1.0;
                cur[c].i = kNone;
            }
            return;
        }
    }
    Best b{-1.0, kNone};
    if (j == 0) {
        double cx = 0.0, cy = 0.0, cz = 0.0;
        bool index_ok = false;
        int s0 = -1;
        if (a.start == PV_FPS_START_INDEX) {
            s0 = a.start_idx[m];
            double x, y, z;
            index_ok = s0 >= 0 && s0 < n && load_point(a.p.points, (int64_t)r.lo + s0, x, y, z);
        } else {
            cx = a.w.cen[m * 3 + 0];
            cy = a.w.cen[m * 3 + 1];
            cz = a.w.cen[m * 3 + 2];
        }
        for (int e = 0; e < kStepPer; ++e) {
            const int i = c * kChunk + t + e * kStepThreads;
            if (i >= n) break;
            double x, y, z, v = -1.0;
            if (load_point(a.p.points, (int64_t)r.lo + i, x, y, z)) {
                if (a.start == PV_FPS_START_INDEX) {
                    v = inf;
                } else {
                    const double key = d2(x, y, z, cx, cy, cz);
                    take(b, key, i);
                    v = a.start == PV_FPS_START_CENTROID_KEPT ? key : inf;
                }
            }
            a.w.md[(int64_t)r.lo + i] = v;
        }
        if (a.start == PV_FPS_START_INDEX && c == 0 && t == 0 && index_ok) take(b, inf, s0);
    } else {
        for (int e = 0; e < kStepPer; ++e) {
            const int i = c * kChunk + t + e * kStepThreads;
            if (i >= n) break;
            double v = a.w.md[(int64_t)r.lo + i];
            if (v < 0.0) continue;
            double x, y, z;
            load_point(a.p.points, (int64_t)r.lo + i, x, y, z);
            const double d = d2(x, y, z, px, py, pz);
            if (d < v) {
                v = d;
                a.w.md[(int64_t)r.lo + i] = v;
            }
            take(b, v, i);
        }
    }
    b = block_best<kStepThreads / 64>(b, slot[1]);
    if (t == 0) {
        cur[c].v = b.v;
        cur[c].i = b.i;
    }
}

// --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_diam_init(unsigned long long *acc, int nmodels) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < nmodels) acc[m] = 0ull;
}

__global__ __launch_bounds__(kTile) void k_diam_pairs(pv_model_points p, unsigned long long *acc, int T) {
    __shared__ double sx[kTile], sy[kTile], sz[kTile];
    __shared__ double sw[kTile / 64];
    // blockIdx.x -> (ti, tj >= ti), rows of the upper triangle one after the other
    const int64_t q = blockIdx.x;
    const double w = 2.0 * T + 1.0;
    int ti = (int)((w - sqrt(w * w - 8.0 * (double)q)) * 0.5);
    ti = ti < 0 ? 0 : ti > T - 1 ? T - 1 : ti;
    auto first = [T](int64_t r) { return r * T - r * (r - 1) / 2; };
    while (ti + 1 < T && first(ti + 1) <= q) ++ti;
    while (ti > 0 && first(ti) > q) --ti;
    const int tj = ti + (int)(q - first(ti));
    if (tj >= T) return;
    const int t = threadIdx.x;
    for (int m = blockIdx.y; m < p.nmodels; m += gridDim.y) {
        const Range r = model_range(p, m);
        if (!r.ok || (int64_t)tj * kTile >= r.n) continue;   // tj >= ti: both tiles lie outside, or only tj
        const int n = r.n, jn = min(kTile, n - tj * kTile);
        const int i = ti * kTile + t, jj = tj * kTile + t;
        double ax = qnan(), ay = qnan(), az = qnan();        // an absent point: every d2 with it is NaN and loses
        if (i < n) {
            double x, y, z;
            if (load_point(p.points, (int64_t)r.lo + i, x, y, z)) ax = x, ay = y, az = z;
        }
        if (t < jn) {
            double x, y, z;
            const bool ok = load_point(p.points, (int64_t)r.lo + jj, x, y, z);
            sx[t] = ok ? x : qnan();
            sy[t] = ok ? y : qnan();
            sz[t] = ok ? z : qnan();
        }
        __syncthreads();
        double best = -1.0;
#pragma unroll 4
        for (int u = 0; u < jn; ++u) {
            const double d = d2(ax, ay, az, sx[u], sy[u], sz[u]);
            best = d > best ? d : best;                      // false for NaN
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double v = __shfl_xor(best, o);
            best = v > best ? v : best;
        }
        if ((t & 63) == 0) sw[t >> 6] = best;
        __syncthreads();
        if (t == 0) {
            for (int v = 1; v < kTile / 64; ++v) best = sw[v] > best ? sw[v] : best;
            // a non-negative double's bits order as it does; + 1 so that 0 means "no pair yet"
            if (best >= 0.0) atomicMax(acc + m, (unsigned long long)__double_as_longlong(best) + 1ull);
        }
        __syncthreads();                                     // sx.. and sw are rewritten for the next model
    }
}

__global__ __launch_bounds__(256) void k_diam_final(const unsigned long long *acc, double *diameter, int nmodels) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= nmodels) return;
    const unsigned long long a = acc[m];
    diameter[m] = a == 0ull ? qnan() : sqrt(__longlong_as_double((long long)(a - 1ull)));
}

// --------------------------------------------------------------------------
int check_points(const pv_model_points *p) {
    if (!p) return PV_EINVAL;
    if (p->nmodels < 0 || p->total < 0 || p->max_pn < 0) return PV_EINVAL;
    return PV_OK;
}

int check_inputs(const pv_model_points *p) {
    if (!p->off || (p->total > 0 && !p->points)) return PV_EINVAL;
    return PV_OK;
}

int check_workspace(const pv_model_points *p, int32_t k, const void *ws, size_t ws_bytes) {
    const size_t need = pv_model_workspace_size(p->nmodels, p->total, k);
    if (need == 0) return PV_EINVAL;
    if (!ws || ws_bytes < need) return PV_EWORKSPACE;
    if ((uintptr_t)ws & 255) return PV_EALIGN;
    return PV_OK;
}

inline int64_t eff_max(const pv_model_points *p) { return std::min<int64_t>(p->max_pn, p->total); }

}  // namespace

extern "C" {

size_t pv_model_workspace_size(int32_t nmodels, int32_t total, int32_t k) {
    if (nmodels < 0 || total < 0 || k < 1 || k > PV_MODEL_MAX_K) return 0;
    return carve(nullptr, nmodels, total).bytes + 256;     // never 0 for good sizes
}

int pv_model_extent(const pv_model_points *p, double *bbox, double *centroid, int32_t *count, pv_stream_t stream) {
    int e = check_points(p);
    if (e) return e;
    if (p->nmodels == 0) return PV_OK;
    if (!bbox && !centroid && !count) return PV_EINVAL;
    if ((e = check_inputs(p))) return e;
    if ((((uintptr_t)bbox | (uintptr_t)centroid) & 7) || ((uintptr_t)count & 3) || ((uintptr_t)p->points & 3) ||
        ((uintptr_t)p->off & 3))
        return PV_EALIGN;
    k_extent<<<dim3((unsigned)p->nmodels), kLanes, 0, (hipStream_t)stream>>>(*p, bbox, centroid, count);
    return last();
}

int pv_farthest_points(const pv_model_points *p, int32_t k, int32_t start, const int32_t *start_idx, int32_t *idx,
                       double *picked, double *pick_d2, void *workspace, size_t workspace_bytes, pv_stream_t stream) {
    int e = check_points(p);
    if (e) return e;
    if (k < 1 || k > PV_MODEL_MAX_K) return PV_EINVAL;
    if (start != PV_FPS_START_CENTROID && start != PV_FPS_START_CENTROID_KEPT && start != PV_FPS_START_INDEX)
        return PV_EINVAL;
    if (p->nmodels == 0) return PV_OK;
    if (!idx || (start == PV_FPS_START_INDEX && !start_idx)) return PV_EINVAL;
    if ((e = check_inputs(p))) return e;
    if ((e = check_workspace(p, k, workspace, workspace_bytes))) return e;
    if ((((uintptr_t)picked | (uintptr_t)pick_d2) & 7) || (((uintptr_t)idx | (uintptr_t)start_idx) & 3) ||
        ((uintptr_t)p->points & 3) || ((uintptr_t)p->off & 3))
        return PV_EALIGN;
    const int64_t cpm = chunks_of(eff_max(p));
    if (cpm > INT32_MAX) return PV_EINVAL;

    hipStream_t st = (hipStream_t)stream;
    FpsArgs a{};
    a.p = *p;
    a.k = k;
    a.start = start;
    a.start_idx = start_idx;
    a.idx = idx;
    a.picked = picked;
    a.pick_d2 = pick_d2;
    a.w = carve(workspace, p->nmodels, p->total);
    a.cpm = (int32_t)cpm;
    if (start != PV_FPS_START_INDEX) {
        k_extent<<<dim3((unsigned)p->nmodels), kLanes, 0, st>>>(*p, nullptr, a.w.cen, a.w.cnt);
        if ((e = last())) return e;
    }
    // the block form also reports every skipped model; its LDS holds the largest model it can meet
    const size_t lds = 2 * (kFpsThreads / 64) * sizeof(Partial) + (size_t)std::min<int64_t>(eff_max(p), kBlockPn) * 12;
    if (lds > 64 * 1024) {
        const hipError_t he = hipFuncSetAttribute((const void *)k_fps_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (he != hipSuccess) return rc(he);
    }
    k_fps_block<<<dim3((unsigned)p->nmodels), kFpsThreads, lds, st>>>(a);
    if ((e = last())) return e;
    if (eff_max(p) > kBlockPn) {
        if (p->nmodels > 65535) return PV_EINVAL;           // the per-step grid's y
        for (int j = 0; j <= k; ++j) {
            a.step = j;
            k_fps_step<<<dim3((unsigned)cpm, (unsigned)p->nmodels), kStepThreads, 0, st>>>(a);
            if ((e = last())) return e;
        }
    }
    return PV_OK;
}

int pv_model_diameter(const pv_model_points *p, double *diameter, void *workspace, size_t workspace_bytes,
                      pv_stream_t stream) {
    int e = check_points(p);
    if (e) return e;
    if (p->nmodels == 0) return PV_OK;
    if (!diameter) return PV_EINVAL;
    if ((e = check_inputs(p))) return e;
    const int64_t T = (eff_max(p) + kTile - 1) / kTile, pairs = T * (T + 1) / 2;
    if (pairs > INT32_MAX) return PV_EINVAL;
    if ((e = check_workspace(p, 1, workspace, workspace_bytes))) return e;
    if (((uintptr_t)diameter & 7) || ((uintptr_t)p->points & 3) || ((uintptr_t)p->off & 3)) return PV_EALIGN;
    const Work w = carve(workspace, p->nmodels, p->total);
    hipStream_t st = (hipStream_t)stream;
    const unsigned mblocks = (unsigned)((p->nmodels + 255) / 256);
    k_diam_init<<<dim3(mblocks), 256, 0, st>>>(w.acc, p->nmodels);
    if ((e = last())) return e;
    if (pairs > 0) {
        k_diam_pairs<<<dim3((unsigned)pairs, (unsigned)std::min(p->nmodels, 65535)), kTile, 0, st>>>(*p, w.acc, (int)T);
        if ((e = last())) return e;
    }
    k_diam_final<<<dim3(mblocks), 256, 0, st>>>(w.acc, diameter, p->nmodels);
    return last();
}

}  // extern "C"
