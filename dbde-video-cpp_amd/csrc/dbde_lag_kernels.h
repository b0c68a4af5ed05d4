// dbde_lag_kernels.h -- launch interface of the lag projections (dbde_hip_project_lag), dbde_lag_kernels.hip.
//
// A lag projection folds the rw x rh window of a batch of frames pixel by pixel over the pairs of frames `lag` apart:
// with (a, b) = (p_{f - lag}, p_f) at the same window pixel, over the counted pairs, product = sum a * b,
// pairsum = sum (a + b), absdiff = sum |b - a|, sqdiff = sum (b - a)^2 (U64 planes) and maxdiff = max |b - a| (a plane
// of the pixel type, 0 where no pair was counted).  Pair f is counted iff f >= max(lead, lag) and frames f and f - lag
// are both accepted.  Validation and the per-chunk payload offsets come from the decode index kernel
// run with the window decoder's chunk geometry (roi_index_geometry), exactly as dbde_hip_project runs it; the launch
// shape and the load pipeline are project_kernel's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_project_kernels.h"

namespace dbde {

// The statistics, one bit each (DBDE_HIP_LAG_*), and all of them.
constexpr uint32_t kLagProduct = 1u, kLagPairSum = 2u, kLagAbsDiff = 4u, kLagSqDiff = 8u, kLagMaxDiff = 16u, kLagAll = 31u;
// The compiled instance that serves a requested mask: 3 (product, pairsum: the autocorrelation's), 28 (absdiff, sqdiff,
// maxdiff: the difference statistics) or 31 (all five).  An instance accumulates all of its statistics and stores the
// requested planes.
constexpr uint32_t kLagInstanceOf(uint32_t stats) { return (stats & ~3u) == 0u ? 3u : (stats & ~28u) == 0u ? 28u : 31u; }
// The largest lag: the slots of the history ring.
constexpr uint32_t kLagMax = 8;
// Frames per pipeline step of lag_kernel.
constexpr uint32_t kLagGroup = 4;
// LDS of one lag_kernel workgroup: the ring (kLagMax slots of one 8-byte decoded (half) row per lane), the
// double-buffered wave totals of a group and the two scalars' wave counts.
constexpr uint32_t kLagLdsBytes = kLagMax * kProjThreads * 8u + 2u * kLagGroup * 2u * (kProjThreads / 64u) * 4u +
                                  2u * (kProjThreads / 64u) * 4u;

struct LagParams {
    const uint8_t *stream;
    const uint64_t *frame_offsets;  // [n_frames]
    uint64_t stream_bytes;          // readable extent of stream
    const uint32_t *chunk_off;      // [n_frames][cpf + 1] from launch_decode_index
    const uint32_t *frame_ok;       // [n_frames]
    uint32_t n_frames;
    int x0, y0, rw, rh;
    uint32_t T;
    uint32_t w;                     // tiles across the frame
    DecGeom geom;                   // the index's chunk geometry (roi_index_geometry)
    uint32_t tx0, ty0;              // the window's first tile column / row
    uint32_t rows, pieces;          // window tile rows; workgroups (of kProjTilesOf(pix) tiles) across one
    uint32_t segments, fps;         // frame segments; frames per segment (the last may hold fewer)
    int accumulate;                 // 1: combine into what the outputs hold
    uint32_t lag, lead;             // 1..kLagMax; frames [0, lead) are history only
    // outputs (segments == 1: written by lag_kernel; otherwise by lag_combine_kernel); NULL = not computed.  The
    // DBDE16 kernels (pix 2) read out_maxdiff as a U16 array.
    uint64_t *out_product, *out_pairsum, *out_absdiff, *out_sqdiff;
    void *out_maxdiff;
    uint64_t *out_pairs, *out_count;
    // per-segment partials [segments][rh * rw] (segments > 1 only), present for the requested statistics: product,
    // pairsum and sqdiff U32 (pix 1) or U64 (pix 2), absdiff U32, maxdiff U8 (pix 1) or U16 (pix 2).
    void *ws_product, *ws_pairsum, *ws_sqdiff;
    uint32_t *ws_absdiff;
    void *ws_maxdiff;
};

// lag_kernel<kLagInstanceOf(stats), pix> (pix: 1 = DBDE, 2 = DBDE16): grid = pieces * rows * segments workgroups of
// kProjThreads; with segments > 1 lag_combine_kernel follows on the same stream.
hipError_t launch_lag(const LagParams &p, uint32_t stats, uint32_t pix, hipStream_t s);
// Bytes of the per-segment partials of a window of `pixels` pixels (0 for one segment), laid out in the order product,
// pairsum, absdiff, sqdiff, maxdiff, each 16-byte aligned, for the statistics of `stats` (the requested ones).
uint64_t lag_workspace_bytes(uint32_t stats, uint32_t segments, uint64_t pixels, uint32_t pix);
// Bytes of one statistic's partials (bit: one of kLag*), rounded up to 16.
uint64_t lag_partial_bytes(uint32_t bit, uint32_t segments, uint64_t pixels, uint32_t pix);

}  // namespace dbde
