// pv_rng.h -- the pipeline's counter RNG: the pixel pairs of the hypotheses
// (rand_index; compact_hyp in pvcompact.hip, item_hyp in pvvote.hip) and the
// downsampling keep decisions (rand_unit; compact_chunk, its look-back
// self-count and compact_hyp's kept).  The reference uses torch's device RNG,
// which cannot be reproduced -- parity tests inject idxs / keep-masks, and
// tests/front_ref.py restates these functions in numpy so that a seeded call
// can be compared with an injected one bit for bit.  Plain C++ with no other
// include, so that a host compiler can build it for tests/test_front_ref.py.
//
// Integer arithmetic throughout but for rand_unit's last step: a 24-bit
// integer converted to float32 (exact) times 2^-24 (exact).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PVV_RNG_HD __host__ __device__
#else
#define PVV_RNG_HD
#endif

namespace pvv __attribute__((visibility("hidden"))) {

// (the fixed-width names need <stdint.h>; these are the same types on every target the library builds for)
static_assert(sizeof(unsigned long long) == 8 && sizeof(unsigned int) == 4 && sizeof(int) == 4, "64 / 32-bit words");

PVV_RNG_HD inline unsigned long long mix64(unsigned long long z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// 32-bit avalanche (lowbias32 constants); two rounds keyed by the seed
PVV_RNG_HD inline unsigned int hash32(unsigned int x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

PVV_RNG_HD inline int rand_index(unsigned long long seed, unsigned long long key, int n) {
    unsigned int r = hash32(hash32((unsigned int)key ^ (unsigned int)seed) + (unsigned int)(key >> 32) + (unsigned int)(seed >> 32));
    return (int)(((unsigned long long)r * (unsigned int)n) >> 32);
}

PVV_RNG_HD inline float rand_unit(unsigned long long seed, unsigned long long key) {
    return (float)(mix64(seed ^ mix64(key ^ 0x5bd1e995ull)) >> 40) * (1.0f / 16777216.0f);
}

}  // namespace pvv
