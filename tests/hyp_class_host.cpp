// pvnet_amd/csrc/pv_hypclass.h compiled for the host (tests/test_hyp_class.py): a hypothesis's class as the
// hypotheses' producers and pv_vote_counts' k_vote_mfma make it.
#include "../pvnet_amd/csrc/pv_hypclass.h"

extern "C" __attribute__((visibility("default"))) void pv_hyp_class_host(const float *hx, const float *hy, int n,
                                                                         unsigned *out) {
    for (int i = 0; i < n; ++i) out[i] = pvv::hyp_class(hx[i], hy[i]);
}

extern "C" __attribute__((visibility("default"))) void pv_hyp_class_consts(float *out3) {
    out3[0] = pvv::kHypMax;
    out3[1] = pvv::kLattice;
    out3[2] = pvv::kMHypMax;
}
