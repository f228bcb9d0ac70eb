// pvnet_amd/csrc/pv_rng.h compiled for the host (tests/test_front_ref.py): the counter RNG's four
// functions over arrays, as the kernels call them.
#include "../pvnet_amd/csrc/pv_rng.h"

#define PV_RNG_EXPORT extern "C" __attribute__((visibility("default")))

PV_RNG_EXPORT void pv_rng_mix64(long long n, const unsigned long long *z, unsigned long long *out) {
    for (long long i = 0; i < n; ++i) out[i] = pvv::mix64(z[i]);
}

PV_RNG_EXPORT void pv_rng_hash32(long long n, const unsigned int *x, unsigned int *out) {
    for (long long i = 0; i < n; ++i) out[i] = pvv::hash32(x[i]);
}

PV_RNG_EXPORT void pv_rng_rand_index(long long n, const unsigned long long *seed, const unsigned long long *key,
                                     const int *m, int *out) {
    for (long long i = 0; i < n; ++i) out[i] = pvv::rand_index(seed[i], key[i], m[i]);
}

PV_RNG_EXPORT void pv_rng_rand_unit(long long n, const unsigned long long *seed, const unsigned long long *key,
                                    float *out) {
    for (long long i = 0; i < n; ++i) out[i] = pvv::rand_unit(seed[i], key[i]);
}
