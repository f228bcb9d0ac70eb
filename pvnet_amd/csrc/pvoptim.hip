// pvoptim.hip -- libpvoptim.so (include/pvoptim.h): the non-finite check and global norm of every
// gradient, the decision whether the step happens (unscale, clip, bias corrections, loss scale), and
// the Adam / AdamW / SGD update with the f16 model copy and the zeroed gradients.  One translation
// unit that includes no other csrc/ file, so the other libraries' sources do not rebuild it.
//
// A block of kThreads lanes takes one chunk of kChunk consecutive elements of one tensor; a lane takes
// groups of 8 consecutive elements, group t, t + kThreads, ... of the chunk:
//   k_optim_stats    gradients -> per chunk (non-finite count, f64 sum of squares) to the workspace
//   k_optim_decide   one block: the partials in a fixed order -> the decision record and the state
//   k_optim_apply    the decision -> master, m, v, the f16 model, zeroed gradients
// Three launches; nothing waits on anything but the stream's order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pvoptim.h"

namespace {

constexpr int kThreads = PV_OPT_THREADS;
constexpr int kGroup = PV_OPT_GROUP;
constexpr int64_t kChunk = PV_OPT_CHUNK;
static_assert(kGroup == 8 && (kThreads & (kThreads - 1)) == 0 && kChunk % (kGroup * kThreads) == 0 &&
                  (kChunk & (kChunk - 1)) == 0,
              "the group accesses below are written for 8 elements, the tree for a power of two");

inline int rc(hipError_t e) { return e == hipSuccess ? PV_OK : (int)e; }
inline int last() { return rc(hipGetLastError()); }
inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// what k_optim_decide leaves for k_optim_apply
struct Decision {
    float k, step_size, sq2, lr, lr_wd;
    int32_t skipped;
};

struct Work {
    double *part_sum;    // [n_chunks]
    uint32_t *part_cnt;  // [n_chunks]
    Decision *dec;
    size_t bytes;
};

// the layout of the workspace; with base == nullptr only the size is wanted and no pointer is formed
inline Work carve(void *base, int64_t n_chunks) {
    Work w{};
    const int64_t o_cnt = align_up(n_chunks * 8, 256);
    const int64_t o_dec = o_cnt + align_up(n_chunks * 4, 256);
    w.bytes = (size_t)(o_dec + align_up((int64_t)sizeof(Decision), 256));
    if (base) {
        char *p = (char *)base;
        w.part_sum = (double *)p;
        w.part_cnt = (uint32_t *)(p + o_cnt);
        w.dec = (Decision *)(p + o_dec);
    }
    return w;
}

struct OptArgs {
    pv_optim_desc d;
    const pv_optim_tensor *table;
    const pv_optim_chunk *chunks;
    pv_optim_state *state;
    Work w;
    int64_t n_chunks;
    int32_t n_tensors;
    float omb1, omb2;    // 1 - beta1, 1 - beta2 in f32
};

// ---- the block's chunk ------------------------------------------------------------------------------
struct Span {
    pv_optim_tensor t;
    int64_t first;
    int len;             // elements of the chunk; 0: nothing to do (also for an entry out of range)
};

__device__ __forceinline__ Span my_span(const OptArgs &a, bool need_v) {
    Span s;
    s.len = 0;
    const pv_optim_chunk c = a.chunks[blockIdx.x];
    if (c.tensor < 0 || c.tensor >= a.n_tensors) return s;
    s.t = a.table[c.tensor];
    s.first = c.first;
    if (c.first < 0 || c.first >= s.t.n || (c.first & (kChunk - 1))) return s;
    if (!s.t.master || !s.t.grad || !s.t.m || (need_v && !s.t.v)) return s;
    if (s.t.grad_kind != PV_OPT_F32 && s.t.grad_kind != PV_OPT_F16) return s;
    const int64_t rest = s.t.n - c.first;
    s.len = (int)(rest < kChunk ? rest : kChunk);
    return s;
}

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ float h2f(uint32_t bits16) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
}
__device__ __forceinline__ uint32_t f2h(float v) {     // round to nearest even
    return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)v);
}

// n <= 8 consecutive elements from p -> f32; 16-byte accesses when vec (then n == 8)
__device__ __forceinline__ void load_f32(const float *p, bool vec, int n, float (&v)[kGroup]) {
    if (vec) {
        const float4 lo = *(const float4 *)p, hi = *(const float4 *)(p + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
        v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    } else {
#pragma unroll
        for (int e = 0; e < kGroup; ++e) v[e] = e < n ? p[e] : 0.f;
    }
}

__device__ __forceinline__ void load_f16(const unsigned short *p, bool vec, int n, float (&v)[kGroup]) {
    if (vec) {
        const uint4 w = *(const uint4 *)p;
        v[0] = h2f(w.x & 0xffffu); v[1] = h2f(w.x >> 16);
        v[2] = h2f(w.y & 0xffffu); v[3] = h2f(w.y >> 16);
        v[4] = h2f(w.z & 0xffffu); v[5] = h2f(w.z >> 16);
        v[6] = h2f(w.w & 0xffffu); v[7] = h2f(w.w >> 16);
    } else {
#pragma unroll
        for (int e = 0; e < kGroup; ++e) v[e] = e < n ? h2f(p[e]) : 0.f;
    }
}

__device__ __forceinline__ void load_grad(const pv_optim_tensor &t, int64_t at, bool vec, int n, float (&g)[kGroup]) {
    if (t.grad_kind == PV_OPT_F32) load_f32((const float *)t.grad + at, vec, n, g);
    else load_f16((const unsigned short *)t.grad + at, vec, n, g);
}

__device__ __forceinline__ void store_f32(float *p, bool vec, int n, const float (&v)[kGroup]) {
    if (vec) {
        *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
        *(float4 *)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int e = 0; e < kGroup; ++e)
            if (e < n) p[e] = v[e];
    }
}

__device__ __forceinline__ void store_f16(unsigned short *p, bool vec, int n, const float (&v)[kGroup]) {
    if (vec) {
        *(uint4 *)p = make_uint4(f2h(v[0]) | (f2h(v[1]) << 16), f2h(v[2]) | (f2h(v[3]) << 16),
                                 f2h(v[4]) | (f2h(v[5]) << 16), f2h(v[6]) | (f2h(v[7]) << 16));
    } else {
#pragma unroll
        for (int e = 0; e < kGroup; ++e)
            if (e < n) p[e] = (unsigned short)f2h(v[e]);
    }
}

__device__ __forceinline__ void zero_grad(const pv_optim_tensor &t, int64_t at, bool vec, int n) {
    const float z[kGroup] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (t.grad_kind == PV_OPT_F32) store_f32((float *)t.grad + at, vec, n, z);
    else store_f16((unsigned short *)t.grad + at, vec, n, z);
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

__device__ __forceinline__ bool finite_f32(float x) {
    return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u;
}

// ---- 1. the gradients' statistics ----------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_optim_stats(OptArgs a) {
    __shared__ double red[kThreads];
    __shared__ uint32_t cnt_s;
    if (threadIdx.x == 0) cnt_s = 0;
    __syncthreads();
    const Span s = my_span(a, false);
    const bool vec = s.len > 0 && aligned16((const char *)s.t.grad + s.first * (s.t.grad_kind == PV_OPT_F32 ? 4 : 2));
    double acc = 0.0;
    uint32_t bad = 0;
    for (int j = threadIdx.x * kGroup; j < s.len; j += kThreads * kGroup) {
        const int n = min(kGroup, s.len - j);
        float g[kGroup];
        load_grad(s.t, s.first + j, vec && n == kGroup, n, g);
#pragma unroll
        for (int e = 0; e < kGroup; ++e) {
            if (e < n) {
                if (finite_f32(g[e])) acc += (double)g[e] * (double)g[e];
                else ++bad;
            }
        }
    }
    if (bad) atomicAdd(&cnt_s, bad);
    block_sum(red, acc);
    if (threadIdx.x == 0) {
        a.w.part_sum[blockIdx.x] = red[0];
        a.w.part_cnt[blockIdx.x] = cnt_s;
    }
}

// ---- 2. the decision -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_optim_decide(OptArgs a) {
    __shared__ double red[kThreads];
    __shared__ uint32_t any_s;
    const int t = threadIdx.x;
    if (t == 0) any_s = 0;
    __syncthreads();
    double acc = 0.0;
    uint32_t bad = 0;
    for (int64_t q = t; q < a.n_chunks; q += kThreads) {
        acc += a.w.part_sum[q];
        bad |= a.w.part_cnt[q];
    }
    if (bad) atomicOr(&any_s, 1u);
    block_sum(red, acc);
    if (t != 0) return;
    pv_optim_state S = *a.state;
    const pv_optim_desc &d = a.d;
    const int found = any_s ? 1 : 0;
    const double inv = 1.0 / (double)S.scale;
    const double norm = sqrt(red[0]) * inv;
    double c = 1.0;
    if (d.max_norm > 0.f) c = fmin(1.0, (double)d.max_norm / (norm + 1e-6));
    Decision dec;
    dec.k = (float)(inv * c);
    if (!found) {
        S.step += 1;
        S.b1pow *= (double)d.beta1;
        S.b2pow *= (double)d.beta2;
    }
    const float bc1 = (float)(1.0 - S.b1pow), bc2 = (float)(1.0 - S.b2pow);
    dec.step_size = S.lr / bc1;
    dec.sq2 = sqrtf(bc2);
    dec.lr = S.lr;
    dec.lr_wd = S.lr * d.weight_decay;
    dec.skipped = found;
    if (d.growth_interval > 0) {
        if (found) {
            S.scale = S.scale * d.backoff_factor;
            S.growth_tracker = 0;
        } else {
            int32_t tr = S.growth_tracker + 1;
            if (tr == d.growth_interval) {
                const float grown = S.scale * d.growth_factor;
                if (finite_f32(grown)) S.scale = grown;
                tr = 0;
            }
            S.growth_tracker = tr;
        }
    }
    S.grad_norm = (float)norm;
    S.found_inf = found;
    S.skipped = found;
    *a.state = S;
    *a.w.dec = dec;
}

// ---- 3. the update -----------------------------------------------------------------------------------------
template <int ALG>
__global__ __launch_bounds__(kThreads) void k_optim_apply(OptArgs a) {
    const Span s = my_span(a, ALG != PV_OPT_SGD);
    if (s.len == 0) return;
    const Decision dec = *a.w.dec;
    const pv_optim_tensor &t = s.t;
    const bool g32 = t.grad_kind == PV_OPT_F32;
    bool vec = aligned16(t.master + s.first) && aligned16(t.m + s.first) &&
               aligned16((const char *)t.grad + s.first * (g32 ? 4 : 2));
    if (ALG != PV_OPT_SGD) vec = vec && aligned16(t.v + s.first);
    if (t.model) vec = vec && aligned16((const unsigned short *)t.model + s.first);
    const float wd = a.d.weight_decay, b1 = a.d.beta1, b2 = a.d.beta2, eps = a.d.eps, mom = a.d.momentum;

    for (int j = threadIdx.x * kGroup; j < s.len; j += kThreads * kGroup) {
        const int n = min(kGroup, s.len - j);
        const bool vg = vec && n == kGroup;
        const int64_t at = s.first + j;
        if (dec.skipped) {
            if (a.d.zero_grads) zero_grad(t, at, vg, n);
            continue;
        }
        float g[kGroup], p[kGroup], m[kGroup], v[kGroup];
        load_grad(t, at, vg, n, g);
        load_f32(t.master + at, vg, n, p);
        load_f32(t.m + at, vg, n, m);
        if (ALG != PV_OPT_SGD) load_f32(t.v + at, vg, n, v);
#pragma unroll
        for (int e = 0; e < kGroup; ++e) {
            float ge = g[e] * dec.k, pe = p[e];
            if (ALG == PV_OPT_SGD) {
                if (wd != 0.f) ge = ge + wd * pe;
                m[e] = mom * m[e] + ge;
                pe = pe - dec.lr * m[e];
            } else {
                if (ALG == PV_OPT_ADAM) {
                    if (wd != 0.f) ge = ge + wd * pe;
                } else {
                    if (wd != 0.f) pe = pe - dec.lr_wd * pe;
                }
                m[e] = b1 * m[e] + a.omb1 * ge;
                v[e] = b2 * v[e] + (a.omb2 * ge) * ge;
                pe = pe - dec.step_size * (m[e] / (sqrtf(v[e]) / dec.sq2 + eps));
            }
            p[e] = pe;
        }
        store_f32(t.master + at, vg, n, p);
        store_f32(t.m + at, vg, n, m);
        if (ALG != PV_OPT_SGD) store_f32(t.v + at, vg, n, v);
        if (t.model) store_f16((unsigned short *)t.model + at, vg, n, p);
        if (a.d.zero_grads) zero_grad(t, at, vg, n);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------
bool alg_ok(int32_t g) { return g == PV_OPT_ADAM || g == PV_OPT_ADAMW || g == PV_OPT_SGD; }
bool fin(float x) { return x == x && x <= 3.0e38f && x >= -3.0e38f; }

int check_desc(const pv_optim_desc *d) {
    if (!d || !alg_ok(d->algorithm)) return PV_EINVAL;
    if (!fin(d->beta1) || !fin(d->beta2) || !fin(d->eps) || !fin(d->weight_decay) || !fin(d->momentum) ||
        !fin(d->growth_factor) || !fin(d->backoff_factor))
        return PV_EINVAL;
    if (d->max_norm != d->max_norm || d->max_norm < -3.0e38f) return PV_EINVAL;   // NaN, -inf
    if (d->beta1 < 0.f || d->beta1 >= 1.f || d->beta2 < 0.f || d->beta2 >= 1.f || !(d->eps > 0.f)) return PV_EINVAL;
    if (d->weight_decay < 0.f || d->momentum < 0.f) return PV_EINVAL;
    if (d->growth_factor < 1.f || !(d->backoff_factor > 0.f) || d->backoff_factor > 1.f) return PV_EINVAL;
    if (d->growth_interval < 0 || (d->zero_grads != 0 && d->zero_grads != 1)) return PV_EINVAL;
    return PV_OK;
}

}  // namespace

extern "C" {

int64_t pv_optim_plan(const pv_optim_tensor *tensors, int32_t count, int32_t algorithm, pv_optim_chunk *chunks,
                      int64_t capacity) {
    if (count < 0 || capacity < 0 || !alg_ok(algorithm) || (count > 0 && !tensors) || (capacity > 0 && !chunks))
        return PV_EINVAL;
    int64_t total = 0;
    for (int32_t i = 0; i < count; ++i) {
        const pv_optim_tensor &t = tensors[i];
        if (t.n < 0 || (t.grad_kind != PV_OPT_F32 && t.grad_kind != PV_OPT_F16)) return PV_EINVAL;
        if (t.n > 0 && (!t.master || !t.grad || !t.m || (algorithm != PV_OPT_SGD && !t.v))) return PV_EINVAL;
        if ((((uintptr_t)t.master | (uintptr_t)t.m | (uintptr_t)t.v) & 3) || ((uintptr_t)t.model & 1) ||
            ((uintptr_t)t.grad & (t.grad_kind == PV_OPT_F32 ? 3 : 1)))
            return PV_EALIGN;
        total += t.n / kChunk + (t.n % kChunk != 0);
        if (total > INT32_MAX) return PV_EINVAL;
    }
    int64_t at = 0;
    for (int32_t i = 0; i < count && at < capacity; ++i)
        for (int64_t first = 0; first < tensors[i].n && at < capacity; first += kChunk) {
            chunks[at].first = first;
            chunks[at].tensor = i;
            chunks[at].pad_ = 0;
            ++at;
        }
    return total;
}

size_t pv_optim_workspace_size(int64_t n_chunks) {
    if (n_chunks < 0 || n_chunks > INT32_MAX) return 0;
    return carve(nullptr, n_chunks).bytes;
}

int pv_optim_step(const pv_optim_desc *d, const pv_optim_tensor *table, int32_t n_tensors, const pv_optim_chunk *chunks,
                  int64_t n_chunks, pv_optim_state *state, void *workspace, size_t workspace_bytes, pv_stream_t stream) {
    const int e0 = check_desc(d);
    if (e0 != PV_OK) return e0;
    if (n_tensors < 0 || n_chunks < 0 || n_chunks > INT32_MAX) return PV_EINVAL;
    if (n_tensors == 0 || n_chunks == 0) return PV_OK;
    if (!table || !chunks || !state) return PV_EINVAL;
    const size_t need = pv_optim_workspace_size(n_chunks);
    if (!workspace || workspace_bytes < need) return PV_EWORKSPACE;
    if (((uintptr_t)workspace & 255) || (((uintptr_t)table | (uintptr_t)chunks | (uintptr_t)state) & 7)) return PV_EALIGN;

    OptArgs a{};
    a.d = *d;
    a.table = table;
    a.chunks = chunks;
    a.state = state;
    a.w = carve(workspace, n_chunks);
    a.n_chunks = n_chunks;
    a.n_tensors = n_tensors;
    a.omb1 = 1.0f - d->beta1;
    a.omb2 = 1.0f - d->beta2;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_chunks);
    int e;
    k_optim_stats<<<grid, kThreads, 0, st>>>(a);
    if ((e = last())) return e;
    k_optim_decide<<<dim3(1), kThreads, 0, st>>>(a);
    if ((e = last())) return e;
    if (d->algorithm == PV_OPT_ADAM) k_optim_apply<PV_OPT_ADAM><<<grid, kThreads, 0, st>>>(a);
    else if (d->algorithm == PV_OPT_ADAMW) k_optim_apply<PV_OPT_ADAMW><<<grid, kThreads, 0, st>>>(a);
    else k_optim_apply<PV_OPT_SGD><<<grid, kThreads, 0, st>>>(a);
    return last();
}

}  // extern "C"
