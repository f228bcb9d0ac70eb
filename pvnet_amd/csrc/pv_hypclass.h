// pv_hypclass.h -- a hypothesis's class for the fused vote/count: a function of
// its two coordinates alone, so the hypotheses' producers (compact_hyp,
// k_hyp_gen) make it once where every wave of k_vote_mfma used to make it again
// for its 128 hypotheses (85 blocks per keypoint on the same 512 values).
// Part of pv_common.h, which includes it; plain C++ with no other include than
// math.h, so that a host compiler can build it for tests/test_hyp_class.py,
// which restates the expressions in numpy float32.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PVV_HYP_HD __host__ __device__
#else
#define PVV_HYP_HD
#endif

namespace pvv __attribute__((visibility("hidden"))) {

// domain of the fast test's error bound
constexpr float kHypMax = 1.0e17f;           // |hx|,|hy| above -> exact-only hypothesis
constexpr float kLattice = 2.5e-6f;          // |h - round(h)| below (both axes) -> exact-only
constexpr float kMHypMax = 8.0e6f;           // k_vote_mfma: |hx|, |hy| from here on -> exact-only (keeps s >= 2^-9)

// Is hypothesis (hx, hy) outside the fast test's domain?  Non-finite, huge, or
// within 2.5e-6 of an integer lattice point (pixel centres are integers, so
// only such hypotheses can come within the reference's norm2 < 1e-6 guard).
PVV_HYP_HD inline bool hyp_exact_only(float hx, float hy) {
    bool big = !(fabsf(hx) <= kHypMax) || !(fabsf(hy) <= kHypMax);   // also NaN/inf
    bool lat = fabsf(hx - rintf(hx)) < kLattice && fabsf(hy - rintf(hy)) < kLattice;
    return big || lat;
}

// k_vote_mfma's class of hypothesis (hx, hy): bit 0 fast (the matrix-core test
// decides its pairs outside the band), bit 1 exact-only (finite, but on the
// lattice or beyond kMHypMax: the reference's sequence decides every pair);
// neither for a non-finite one, which is never an inlier.
constexpr uint32_t kHypFast = 1u, kHypExact = 2u;
PVV_HYP_HD inline uint32_t hyp_class(float hx, float hy) {
    const bool fin = __builtin_isfinite(hx) && __builtin_isfinite(hy);
    const bool xo = fin && (hyp_exact_only(hx, hy) || !(fabsf(hx) < kMHypMax && fabsf(hy) < kMHypMax));
    return (fin && !xo ? kHypFast : 0u) | (xo ? kHypExact : 0u);
}

}  // namespace pvv
