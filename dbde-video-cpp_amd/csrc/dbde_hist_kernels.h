// dbde_hist_kernels.h -- launch interface of the per-frame intensity histograms (dbde_hip_histogram),
// dbde_hist_kernels.hip.
//
// A histogram counts the pixels of the rw x rh window of each frame of a batch by value: pixel v goes to bin
// min(v >> shift, bins - 1).  Validation and the per-chunk payload offsets come from the decode index kernel run with
// the window decoder's chunk geometry (roi_index_geometry), exactly as dbde_hip_project runs it; the histogram kernel
// reads the window's tiles with the projection's lane mapping and counts them in LDS, writing no image.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"

namespace dbde {

// A piece is kHistTilesOf(pix) consecutive tiles of one window tile row: one lane per tile row (pix 1: 8 lanes per
// tile) or per half tile row (pix 2, DBDE16: 16 lanes per tile), as the projection kernel maps them.  A workgroup
// takes one segment (a run of consecutive pieces) of one frame.
constexpr uint32_t kHistThreads = 256;
constexpr uint32_t kHistTilesOf(uint32_t pix) { return kHistThreads / (8u * pix); }
constexpr uint32_t kHistWaves = kHistThreads / 64u;
// Threads per workgroup of the init kernel (one output bin per thread).
constexpr uint32_t kHistRowThreads = 256;
// The LDS histogram of a kernel instance: up to 256 bins with one copy per wave, or up to 4,096 bins (DBDE16) with one
// copy shared by the workgroup.
constexpr uint32_t kHistSmallBins = 256, kHistLargeBins = 4096;
constexpr uint32_t kHistLdsBinsOf(uint32_t bins) { return bins <= kHistSmallBins ? kHistSmallBins : kHistLargeBins; }
constexpr uint32_t kHistCopiesOf(uint32_t lds_bins) { return lds_bins <= kHistSmallBins ? kHistWaves : 1u; }
// Frames of the pipeline step (pieces in flight per step) and the offsets scan's LDS: 2 x G x 2 x waves words.
constexpr uint32_t kHistGroup = 4;
constexpr uint32_t kHistLdsBytesOf(uint32_t lds_bins) {
    return 4u * kHistCopiesOf(lds_bins) * lds_bins + 4u * 2u * kHistGroup * 2u * kHistWaves;
}

struct HistParams {
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
    uint32_t rows, pieces;          // window tile rows; pieces across one
    uint32_t segments, pps;         // workgroups per frame; pieces per segment (the last may hold fewer)
    uint32_t shift, bins;
    int accumulate;                 // 1: add to out_total / out_count
    // outputs; NULL = not computed.  out_hist [n_frames][bins] U32; out_total [bins] U64, out_count one U64.
    uint32_t *out_hist;
    uint64_t *out_total, *out_count;
};

// hist_init_kernel (the accepted frames' rows to 0; with accumulate = 0 the total and count to 0), then, for
// n_frames > 0, hist_kernel<pix, kHistLdsBinsOf(bins)> (grid = n_frames * segments workgroups of kHistThreads).
// Rejected frames' rows are never written.  pix: 1 = DBDE, 2 = DBDE16.
hipError_t launch_histogram(const HistParams &p, uint32_t pix, hipStream_t s);

}  // namespace dbde
