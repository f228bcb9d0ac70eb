// pv_tunables.h -- every numeric default of the voting library that a build
// may override (tools/build_variant.py NAME -DMACRO=V passes its defines to
// every translation unit), each with the measurement behind it.  One place,
// so that the kernels and pv_build_config() (pvpipeline.hip) cannot disagree.
// DESIGN.md section 7 has the A/B records; the variants measured and removed
// are in DESIGN.md's appendix "Removed variants".
#pragma once

// ---- k_refine_solve --------------------------------------------------------
// refine blocks per (image, keypoint); measured with the gathering hand-off
// (tools/ab_libs.sh, two rounds, stream images/s and sequential latency):
// 16 -> 53.8-54.0k / 47.7-48.6 us, 32 -> 53.2-53.3k / 47.5-48.2 us; with the
// round-4 ticket hand-off 8 -> 52.7k / 50.9-51.8 us, 16 -> 53.0k / 50.8-51.2,
// 32 -> 52.5-52.7k / 51.1-51.6 (the round-4 kernel itself: 52.5-52.7k / 52.1)
#ifndef PVV_REFINE_NJ
#define PVV_REFINE_NJ 16
#endif
// refine block threads (round 5, 16 blocks per keypoint: 256 -> 53.6-53.9k
// images/s, 512 -> 52.7-53.6k, 1024 -> 44.5k / 50.5 us; round 4, same threads
// per keypoint: 8 x 256 43.3-43.8k / 51.9 us, 16 x 128 43.0k / 53.6-53.9 us,
// 32 x 64 41.6k / 59.5 us)
#ifndef PVV_REFINE_T
#define PVV_REFINE_T 256
#endif

// ---- k_fg_count ------------------------------------------------------------
// one-chunk blocks in the grid above which k_fg_count runs its wide form
// (8 chunks per block); the measurements are in k_fg_count's head comment
#ifndef PVV_FG_WIDE_ABOVE
#define PVV_FG_WIDE_ABOVE 4096
#endif

// ---- k_vote_mfma (the matrix-core vote) -------------------------------------
// pixels per sub-chunk: a unit's range (~350 px at configs[1]) in one; 352
// (with a 128-entry band queue) keeps the block's LDS under 40 KiB, so a
// fourth block -- the next image's -- fits beside a launch's three per CU
#ifndef PVM_CHUNK
#define PVM_CHUNK 352
#endif
// band pairs queued per wave before a reference pass
#ifndef PVM_QUEUE
#define PVM_QUEUE 128
#endif
// waves per SIMD the registers are sized for.  Round 2: 3 (152 VGPRs; 4 then
// spilled across the hot loop): 40.4k -> 41.5k images/s.  Round 6: the kernel
// needs 129 at 3 -- one over the 128 that lets a fourth wave, the next
// frame's block, share the SIMD -- and fits 122 without spills at 4: the
// batch-1 stream 53.2-53.5k -> 54.2-54.6k images/s, latency unchanged
// (profiles/r06/vote_wpe_ab.txt)
#ifndef PVM_WPE
#define PVM_WPE 4
#endif
// k_vote_mfma blocks per CU (tools/vm_ab.sh, 8 in flight: 4 -> 36.6k images/s,
// 3 -> 40.2k, 2 -> 39.7k)
#ifndef PVV_VM_BPC
#define PVV_VM_BPC 3
#endif
static_assert(PVV_VM_BPC >= 1 && PVV_VM_BPC <= 4, "k_vote_mfma: 1..4 blocks per CU");

// ---- k_vote_bytes (the byte-mask vote) --------------------------------------
// hypothesis records per batch (rows per wave, <= 64)
#ifndef PVV_BYTE_HB
#define PVV_BYTE_HB 64
#endif
// XCD-contiguous item ranges (31.1 vs 31.9 us interleaved)
#ifndef PVV_BYTES_XCD
#define PVV_BYTES_XCD 1
#endif
// CU-balanced grid of full + quarter blocks (33.0 -> 31.1 us)
#ifndef PVV_BYTES_BAL
#define PVV_BYTES_BAL 1
#endif
