// pv_band.h -- the per-launch constants of k_vote_mfma's band re-check
// (pvvote.hip): functions of tau, gzf and gzr
// alone, made once on the host when VoteArgs is filled instead of in every
// lane of every wave for every sub-chunk (two divisions).  Plain C++ with no
// other include, so that a host compiler can build it for
// tests/test_band_consts.py, which restates the expressions in numpy float32.
//
// Every operation is a float32 one, rounded by itself (-ffp-contract=off; the
// device's divisions are correctly rounded, pvnet_amd/build.py): the host
// makes the values the kernel used to make, bit for bit.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PVV_BAND_HD __host__ __device__
#else
#define PVV_BAND_HD
#endif

namespace pvv __attribute__((visibility("hidden"))) {

struct BandConsts {
    float kx, ky;   // round 5's per-pair bound g = G + kx |X| + ky |Y| (what the filter below contains)
    float inv1k;    // 1.0002 / (1 - 1.0001 ky): ky reaches 8e-4 at thr 0.999999 (gzr grows with 1 / tau)
    float gq;       // a set's G' = gb gq, from the hot loop's bound gb = (gzf + gzr) B s 1.00001
    float Kb;       // K = (kx + ky) inv1k of the one-FMA filter t = |z| - K |X| <= G'
};

PVV_BAND_HD inline BandConsts band_consts(float tau, float gzf, float gzr) {
    BandConsts k;
    k.kx = gzr / tau * 1.0001f;
    k.ky = gzr * 1.0001f;
    k.inv1k = 1.0002f / (1.f - k.ky * 1.0001f);
    k.gq = gzf / (gzf + gzr) * 1.0011f * k.inv1k;
    k.Kb = (k.kx + k.ky) * k.inv1k;
    return k;
}

}  // namespace pvv
