// pvpipeline.hip -- the voting pipeline of libpvvote.so and the general part of
// its C ABI (include/pvvote.h).  Host code only: front_half (compaction,
// hypotheses, fused vote/count) and the v3 / v5 / motion / EVD entries launch
// each stage through its launcher in pv_stages.h; beside them the version,
// build-config, error-string, device and stream entries, the workspace size
// and launch count, and the profiling builds' ablation mask.  pvvote.hip's
// head comment maps the library's files.
#include "pv_stages.h"

#define PV_VERSION "pvvote 0.2 (gfx950)"

#ifdef PVV_PROFILE
namespace pvv __attribute__((visibility("hidden"))) {
// pv_debug_set_ablation (pv_stages.h lists the bits); -DPVV_ABL_DEFAULT=M starts a
// profiling build with mask M, for counter passes over a program that sets none
#ifndef PVV_ABL_DEFAULT
#define PVV_ABL_DEFAULT 0
#endif
int g_abl = PVV_ABL_DEFAULT;
}
#endif

namespace {

using namespace pvv;

int check_desc(const pv_image_desc *img) {
    if (!img || !img->mask || !img->vertex) return PV_EINVAL;
    if (img->b <= 0 || img->H <= 0 || img->W <= 0 || img->vn <= 0 || img->vn > 64) return PV_EINVAL;
    if (img->H > 65535 || img->W > 65535) return PV_EINVAL;   // pixel centres pack into 16 bits
    if (img->mask_kind < PV_MASK_I64 || img->mask_kind > PV_MASK_SEG_F16) return PV_EINVAL;
    if (img->vertex_kind != PV_VERTEX_F32 && img->vertex_kind != PV_VERTEX_F16) return PV_EINVAL;
    if (img->ncls < 0 || img->ncls > 64) return PV_EINVAL;
    if ((int64_t)img->b * std::max(img->ncls, 1) > INT32_MAX) return PV_EINVAL;
    return PV_OK;
}

// the images the pipeline's stages after k_label_count see: one per (image,
// class) of a multi-object call (the virtual image bv = bi * ncls + c)
int pipeline_images(const pv_image_desc *img) { return img->b * std::max(img->ncls, 1); }

// The mask and vertex views of a call's images.  extent is left 0: front_half
// works it out (the compaction's buffer loads need it), the motion path never
// reads it.
void image_views(const pv_image_desc *img, MaskView *m, VertexView *vx) {
    *m = MaskView{img->mask, img->mask_strides[0], img->mask_strides[1], img->mask_strides[2], img->mask_strides[3]};
    vx->p = img->vertex;
    vx->kind = img->vertex_kind;
    for (int i = 0; i < 5; ++i) vx->s[i] = img->vertex_strides[i];
    vx->extent = 0;
    vx->ncls = img->ncls;
    vx->cs = (int64_t)img->vn * img->vertex_strides[3];
}

// The vote kernels index their work in 32 bits: the vote units of one image
// if every pixel were foreground (0: too many, the call is refused) ...
int64_t vote_units_per_image(int vn, int nh, int64_t P) {
    const int64_t per_img = (int64_t)vn * ((nh + kGroup - 1) / kGroup) * P;
    return per_img >= (1ll << 31) ? 0 : per_img;
}
// ... and the images per vote launch such that this upper bound stays < 2^31
int images_per_vote_launch(int b, int64_t per_img) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(b, ((1ll << 31) - 1) / per_img));
}
// the hypotheses by k_compact's first blocks (compact_hyp) instead of a k_hyp_gen launch
bool hyp_fused(int nh, int nblk) { return hyp_pregen_used(nh) && nblk <= kHypMaxChunks; }

// compaction + hypotheses + fused vote/count, shared by v3 and EVD
int front_half(const pv_image_desc *img, const pv_vote_params *prm, int nh, bool evd, const Workspace &w,
               const pv_v3_diag &dg, hipStream_t s) {
    const int b = pipeline_images(img), H = img->H, W = img->W, vn = img->vn;
    const int64_t P = (int64_t)H * W;
    const int nblk = (int)((P + kCompactChunk - 1) / kCompactChunk);
    CompactArgs ca;
    ca.ncls = img->ncls;
    ca.mask_kind = img->mask_kind;
    ca.evd = evd;
    image_views(img, &ca.m, &ca.vx);
    {   // bytes one image's view spans (the compaction's buffer-load range)
        const int64_t es = img->vertex_kind == PV_VERTEX_F32 ? 4 : 2;
        int64_t hi = 0;
        const int64_t dims[5] = {1, H, W, (int64_t)vn * std::max(img->ncls, 1), 2};   // the whole image view
        for (int i = 1; i < 5; ++i) {
            if (ca.vx.s[i] < 0) return PV_EINVAL;
            hi += (dims[i] - 1) * ca.vx.s[i];
        }
        if ((hi + 1) * es > INT32_MAX) return PV_EINVAL;
        ca.vx.extent = (int32_t)((hi + 1) * es);
    }
    ca.b = b; ca.H = H; ca.W = W; ca.vn = vn; ca.nblk = nblk;
    ca.min_num = prm->min_num; ca.max_num = prm->max_num;
    ca.seed = mix64(prm->seed ^ 0xd1b54a32d192ed03ull);
    ca.keep = prm->keep;
    ca.ws = w;
    ca.s = s;
    const int64_t per_img = vote_units_per_image(vn, nh, P);
    if (!per_img) return PV_EINVAL;
    const bool hfuse = hyp_fused(nh, nblk) && !(g_abl & 2);
    ca.hg = HypGen{};
    if (hfuse) {
        ca.hg.nhb = (int)(((int64_t)nh * vn + 255) / 256);
        ca.hg.nh = nh; ca.hg.vn = vn; ca.hg.min_num = prm->min_num; ca.hg.max_num = prm->max_num;
        ca.hg.seed = mix64(prm->seed); ca.hg.kseed = ca.seed;
        ca.hg.idxs = prm->idxs; ca.hg.keep = prm->keep;
        ca.hg.hyp_out = w.hyp; ca.hg.hypv_out = w.hypv; ca.hg.hypcls = w.hypcls; ca.hg.diag_hyp = dg.hyp;
        ca.hg.keptbits = w.keptbits;
    }
    int r = compact(ca);
    if (r) return r;
    if (dg.ev_compact_end) {
        hipError_t e = hipEventRecord((hipEvent_t)dg.ev_compact_end, s);
        if (e != hipSuccess) return rc(e);
    }
    VoteArgs va{};
    va.pex = w.pex; va.P = (int32_t)P;
    va.hyp = nullptr;
    va.hyp_out = w.hyp; va.diag_hyp = dg.hyp;
    va.idxs = prm->idxs; va.seed = mix64(prm->seed);
    va.counts = w.counts; va.cnt_bs = vn * nh; va.cnt_v = nh; va.cnt_h = 1;
    va.tn_dev = w.tn; va.tn_host = 0;
    va.b = b; va.vn = vn; va.nh = nh; va.hgn = (nh + kGroup - 1) / kGroup;
    fast_constants(prm->inlier_thresh, &va);
    // k_vote_count generates the hypotheses itself (item_hyp in its
    // prologue, overlapped with its first pixel loads) and stores them in
    // the reference layout; k_vote_mfma (hyp_pregen) reads them keypoint-major
    // with their classes (w.hypcls), made before it by k_compact's first
    // blocks or, above kHypMaxChunks, by one k_hyp_gen launch
    if (hyp_pregen_used(nh)) {
        va.hypv_out = w.hypv;
        va.hypcls = w.hypcls;
        if (!hfuse) launch_hyp_gen(va, s);
        if ((r = last())) return r;
        va.hyp = w.hypv; va.hyp_sb = (int64_t)vn * nh; va.hyp_sv = nh; va.hyp_sh = 1;
    }
    if (dg.ev_vote_begin) {
        hipError_t e = hipEventRecord((hipEvent_t)dg.ev_vote_begin, s);
        if (e != hipSuccess) return rc(e);
    }
    const int chunk = images_per_vote_launch(b, per_img);
    for (int b0 = 0; b0 < b; b0 += chunk) {
        VoteArgs vc = va;
        const int nb = std::min(chunk, b - b0);
        vc.b = nb;
        vc.b0 = b0;
        vc.pex += (int64_t)b0 * vn * P;
        vc.hyp_out += (int64_t)b0 * nh * vn;
        if (vc.hyp) vc.hyp += (int64_t)b0 * nh * vn;
        if (vc.hypcls) vc.hypcls += (int64_t)b0 * vn * hyp_sets(nh) * 2;
        if (vc.diag_hyp) vc.diag_hyp += (int64_t)b0 * nh * vn * 2;
        if (vc.idxs) vc.idxs += (int64_t)b0 * nh * vn * 2;
        vc.counts += (int64_t)b0 * va.cnt_bs;
        vc.tn_dev += b0;
        if (!(g_abl & 4) && (r = launch_pipeline_vote(vc, nb * per_img, s))) return r;
        if ((r = last())) return r;
    }
    if (dg.ev_vote_end) return rc(hipEventRecord((hipEvent_t)dg.ev_vote_end, s));
    return PV_OK;
}

}  // namespace


// ==========================================================================
// C ABI
// ==========================================================================
extern "C" {

const char *pv_version(void) { return PV_VERSION; }

#define PVV_STR2(x) #x
#define PVV_STR(x) PVV_STR2(x)
const char *pv_build_config(void) {
    // (band, rw, hypgen, hypfuse, fg_cpb, compact_skip: switches since fixed, kept
    // as literals so that bench records stay comparable across rounds)
    return "vote=k_vote_mfma(bpc=" PVV_STR(PVV_VM_BPC) ",wpe=" PVV_STR(PVM_WPE) ",chunk=" PVV_STR(PVM_CHUNK) ",queue=" PVV_STR(PVM_QUEUE) ",band=2,rw=0/0/0)"
           " hypgen=1 hypfuse=1"
           " refine=" PVV_STR(PVV_REFINE_NJ) "x" PVV_STR(PVV_REFINE_T)
           " fg_cpb=1/8 compact_skip=1"
           " bytes=k_vote_bytes(rows=" PVV_STR(PVV_BYTE_HB) ",xcd=" PVV_STR(PVV_BYTES_XCD) ",bal=" PVV_STR(PVV_BYTES_BAL) ")"
#ifdef PVV_TRACE
           " TRACE"
#endif
#ifdef PVV_PROFILE
           " PROFILE"
#endif
        ;
}

const char *pv_error_string(int code) {
    switch (code) {
    case PV_OK: return "ok";
    case PV_EINVAL: return "invalid argument";
    case PV_EWORKSPACE: return "workspace missing or too small";
    case PV_EALIGN: return "misaligned pointer";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

int pv_device_arch(char *buf, int len) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return rc(e);
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return rc(e);
    if (buf && len > 0) {
        strncpy(buf, prop.gcnArchName, (size_t)len - 1);
        buf[len - 1] = 0;
    }
    return PV_OK;
}

int pv_stream_create(int32_t priority, pv_stream_t *out) {
    if (!out) return PV_EINVAL;
    hipStream_t s = nullptr;
    const hipError_t e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority);
    if (e != hipSuccess) return rc(e);
    *out = (pv_stream_t)s;
    return PV_OK;
}

int pv_stream_destroy(pv_stream_t stream) {
    if (!stream) return PV_EINVAL;
    return rc(hipStreamDestroy((hipStream_t)stream));
}

int pv_stream_capture_id(pv_stream_t stream, uint64_t *id) {
    if (!id) return PV_EINVAL;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    const hipError_t e = hipStreamGetCaptureInfo((hipStream_t)stream, &st, &cid);
    if (e != hipSuccess) return rc(e);
    *id = st == hipStreamCaptureStatusActive ? (uint64_t)cid : 0;
    return PV_OK;
}

#ifdef PVV_PROFILE
// profiling builds only (never during a capture): work left out of the next
// launches (g_abl's bits); outputs are wrong
int pv_debug_set_ablation(int32_t m) {
    g_abl = m;
    return PV_OK;
}
#endif

size_t pv_v3_workspace_size(int32_t b, int32_t H, int32_t W, int32_t vn, int32_t n_hyp) {
    if (b <= 0 || H <= 0 || W <= 0 || vn <= 0 || n_hyp <= 0) return 0;
    return carve(nullptr, b, H, W, vn, n_hyp).total;
}

int pv_v3_kernel_launches(int32_t b, int32_t H, int32_t W, int32_t vn, int32_t n_hyp) {
    if (b <= 0 || H <= 0 || W <= 0 || vn <= 0 || n_hyp <= 0) return 0;
    const int64_t P = (int64_t)H * W;
    const int nblk = (int)((P + kCompactChunk - 1) / kCompactChunk);
    const int64_t per_img = vote_units_per_image(vn, n_hyp, P);
    if (!per_img) return 0;
    const int chunk = images_per_vote_launch(b, per_img);
    const bool pre = hyp_pregen_used(n_hyp);
    return 2 + (pre && !hyp_fused(n_hyp, nblk) ? 1 : 0) + (b + chunk - 1) / chunk + 1;
}

int pv_ransac_voting_v3(const pv_image_desc *img, const pv_vote_params *prm, float *out, void *workspace,
                        size_t workspace_bytes, const pv_v3_diag *diag, pv_stream_t stream) {
    int r = check_desc(img);
    if (r) return r;
    if (!prm || !out || prm->round_hyp_num <= 0) return PV_EINVAL;
    const int nh = prm->round_hyp_num;
    Workspace w = carve(workspace, pipeline_images(img), img->H, img->W, img->vn, nh);
    if (!workspace || workspace_bytes < w.total) return PV_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    pv_v3_diag dg{};
    if (diag) dg = *diag;
    if ((r = front_half(img, prm, nh, false, w, dg, s))) return r;
    const int b = pipeline_images(img), vn = img->vn;
    const int64_t P = (int64_t)img->H * img->W;
    if (!(g_abl & 8)) launch_refine(w, hyp_pregen_used(nh), b, vn, nh, P, prm, out, dg, s);
    if ((r = last())) return r;
    if (dg.counts) {
        hipError_t e = hipMemcpyAsync(dg.counts, w.counts, sizeof(int32_t) * (size_t)b * vn * nh,
                                      hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return rc(e);
    }
    return PV_OK;
}

int pv_ransac_voting_v5(const pv_image_desc *img, const pv_vote_params *prm, float conf_thresh, float *out,
                        float *conf, void *workspace, size_t workspace_bytes, const pv_v3_diag *diag,
                        pv_stream_t stream) {
    if (!conf) return PV_EINVAL;
    int r = pv_ransac_voting_v3(img, prm, out, workspace, workspace_bytes, diag, stream);
    if (r) return r;
    Workspace w = carve(workspace, pipeline_images(img), img->H, img->W, img->vn, prm->round_hyp_num);
    const int64_t P = (int64_t)img->H * img->W;
    launch_point_conf(w, out, pipeline_images(img), img->vn, P, conf_thresh, conf, (hipStream_t)stream);
    return last();
}

int pv_ransac_motion_voting(const pv_image_desc *img, float *out, pv_stream_t stream) {
    int r = check_desc(img);
    if (r) return r;
    if (!out || img->mask_kind == PV_MASK_SEG_F32 || img->mask_kind == PV_MASK_SEG_F16) return PV_EINVAL;
    if (img->ncls > 0) return PV_EINVAL;   // one object per image only
    hipStream_t s = (hipStream_t)stream;
    const int b = img->b, vn = img->vn;
    // stream-ordered, zeroed scratch: sums [b][vn][2] f64, counts [b], tickets [b]
    const size_t acc_bytes = sizeof(double) * 2 * (size_t)b * vn, bytes = acc_bytes + sizeof(int32_t) * 2 * b;
    char *scr = nullptr;
    hipError_t e = hipMallocAsync((void **)&scr, bytes, s);
    if (e != hipSuccess) return rc(e);
    e = hipMemsetAsync(scr, 0, bytes, s);
    if (e != hipSuccess) return rc(e);
    MaskView m;
    VertexView vx;
    image_views(img, &m, &vx);
    int32_t *cnt = (int32_t *)(scr + acc_bytes);
    r = launch_motion(img->mask_kind, m, vx, b, img->H, img->W, vn, (double *)scr, cnt, cnt + b, out, s);
    if (r) return r;
    r = last();
    e = hipFreeAsync(scr, s);
    return r ? r : rc(e);
}

static int evd_front(const pv_image_desc *img, const pv_vote_params *prm, void *workspace, size_t workspace_bytes,
                     Workspace *w, int *nh, hipStream_t s, const pv_v3_diag *diag = nullptr) {
    int r = check_desc(img);
    if (r) return r;
    if (!prm || prm->round_hyp_num <= 0 || prm->min_hyp_num <= 0) return PV_EINVAL;
    int rounds = (prm->min_hyp_num + prm->round_hyp_num - 1) / prm->round_hyp_num;
    *nh = rounds * prm->round_hyp_num;
    *w = carve(workspace, pipeline_images(img), img->H, img->W, img->vn, *nh);
    if (!workspace || workspace_bytes < w->total) return PV_EWORKSPACE;
    pv_v3_diag ev{};     // the diag's timing events only (bench.py's U4 line)
    if (diag) {
        ev.ev_vote_begin = diag->ev_vote_begin;
        ev.ev_vote_end = diag->ev_vote_end;
        ev.ev_compact_end = diag->ev_compact_end;
    }
    return front_half(img, prm, *nh, true, *w, ev, s);
}

int pv_estimate_voting_distribution_with_mean_diag(const pv_image_desc *img, const pv_vote_params *prm,
                                                   const float *mean, float *cov, void *workspace,
                                                   size_t workspace_bytes, const pv_v3_diag *diag,
                                                   pv_stream_t stream) {
    if (!mean || !cov) return PV_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    int nh = 0;
    int r = evd_front(img, prm, workspace, workspace_bytes, &w, &nh, s, diag);
    if (r) return r;
    launch_evd_with_mean(w, pipeline_images(img), img->vn, nh, prm->min_num, prm->min_hyp_num, mean, cov, s);
    return last();
}

int pv_estimate_voting_distribution_with_mean(const pv_image_desc *img, const pv_vote_params *prm,
                                              const float *mean, float *cov, void *workspace,
                                              size_t workspace_bytes, pv_stream_t stream) {
    return pv_estimate_voting_distribution_with_mean_diag(img, prm, mean, cov, workspace, workspace_bytes, nullptr,
                                                          stream);
}

int pv_estimate_voting_distribution(const pv_image_desc *img, const pv_vote_params *prm, float *mean, float *cov,
                                    void *workspace, size_t workspace_bytes, pv_stream_t stream) {
    if (!mean || !cov || !prm || prm->topk <= 0) return PV_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    int nh = 0;
    int r = evd_front(img, prm, workspace, workspace_bytes, &w, &nh, s);
    if (r) return r;
    launch_evd_topk(w, pipeline_images(img), img->vn, nh, prm->min_num, prm->topk, mean, cov, s);
    return last();
}

}  // extern "C"
