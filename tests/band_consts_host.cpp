// pvnet_amd/csrc/pv_band.h compiled for the host (tests/test_band_consts.py): the constants of
// k_vote_mfma's band re-check as launch_vote makes them for VoteArgs.
#include "../pvnet_amd/csrc/pv_band.h"

extern "C" __attribute__((visibility("default"))) void pv_band_consts_host(float tau, float gzf, float gzr, float *out5) {
    const pvv::BandConsts k = pvv::band_consts(tau, gzf, gzr);
    out5[0] = k.kx;
    out5[1] = k.ky;
    out5[2] = k.inv1k;
    out5[3] = k.gq;
    out5[4] = k.Kb;
}
