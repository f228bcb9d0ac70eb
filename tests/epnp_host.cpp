// epnp_host.cpp -- pvnet_amd/csrc/pvepnp_core.h compiled for the host (plain C++, no HIP): the
// kernel's lane phases run as loops over the 64 lanes, so the arithmetic of pv_epnp can be checked
// against tests/epnp_ref.py without a device.  TEST INFRASTRUCTURE ONLY: tests/test_epnp_core_host.py
// builds this file with the host compiler into a scratch directory.
#include <string.h>

#include "../pvnet_amd/csrc/pvepnp_core.h"

extern "C" int pv_epnp_host(int pn, const double *p3, const double *K, const float *p2f, const double *p2d,
                            double *Rt, double *rt6, double *cand_err, int *n_used) {
    if (pn < pve::kMinPts || pn > pve::kMaxPts || (!p2f && !p2d)) return -1;
    pve::Epnp *S = new pve::Epnp;
    memset(S, 0xff, sizeof *S);   // LDS starts undefined on the device: NaN bit patterns here
    pve::Out o;
    pve::epnp_image(*S, pn, p3, K, p2d ? nullptr : p2f, p2d, o);
    delete S;
    memcpy(Rt, o.Rt, sizeof o.Rt);
    memcpy(rt6, o.rt6, sizeof o.rt6);
    memcpy(cand_err, o.cand_err, sizeof o.cand_err);
    *n_used = o.n_used;
    return o.status;
}
