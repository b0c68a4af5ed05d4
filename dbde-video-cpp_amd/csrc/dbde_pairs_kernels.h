// dbde_pairs_kernels.h -- launch interface of the neighbour-product projections (dbde_hip_project_pairs),
// dbde_pairs_kernels.hip.
//
// A pair projection folds the rw x rh window of a batch of frames into one U64 plane per requested forward offset
// (dx, dy) in {(+1, 0), (0, +1), (+1, +1), (-1, +1)}: out[j][y][x] = sum over the accepted frames of
// p[y][x] * p[y + dy][x + dx] where both pixels lie inside the window.  Validation and the per-chunk
// payload offsets come from the decode index kernel run with the window decoder's chunk geometry
// (roi_index_geometry), exactly as dbde_hip_project runs it; the launch shape and the load pipeline are
// project_kernel's, with overlapping pieces and a second prefix for the tile row below (the halo).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_project_kernels.h"

namespace dbde {

// The offsets, one bit each (DBDE_HIP_PAIR_*), and all of them.
constexpr uint32_t kPairRight = 1u, kPairDown = 2u, kPairDownRight = 4u, kPairDownLeft = 8u, kPairAll = 15u;
// The compiled instance that serves a requested mask: 1 (RIGHT alone: no row below), 3 (RIGHT, DOWN) or 15 (all four).
// An instance accumulates all of its offsets and stores the requested planes.
constexpr uint32_t kPairsInstanceOf(uint32_t pairs) { return pairs == 1u ? 1u : (pairs & ~3u) == 0u ? 3u : 15u; }
// Halo tiles of a piece: a workgroup decodes kProjTilesOf(pix) tiles and owns the pairs whose first pixel lies in all
// but its first kPairsHaloLeft (DOWN_LEFT reaches into the tile before) and its last kPairsHaloRight (RIGHT and
// DOWN_RIGHT reach into the tile after); the window's first piece has no left halo and its last no right one.
constexpr uint32_t kPairsHaloLeft(uint32_t inst) { return (inst & kPairDownLeft) ? 1u : 0u; }
constexpr uint32_t kPairsHaloRight(uint32_t inst) { return (inst & (kPairRight | kPairDownRight)) ? 1u : 0u; }
// Tiles between the first tiles of two neighbouring pieces.
constexpr uint32_t kPairsStrideOf(uint32_t inst, uint32_t pix) {
    return kProjTilesOf(pix) - kPairsHaloLeft(inst) - kPairsHaloRight(inst);
}
// Pieces across a window of ntx tiles: one while it fits a workgroup, then one more per stride.
constexpr uint32_t kPairsPiecesOf(uint32_t ntx, uint32_t inst, uint32_t pix) {
    return ntx <= kProjTilesOf(pix) ? 1u : 1u + (ntx - kProjTilesOf(pix) + kPairsStrideOf(inst, pix) - 1u) / kPairsStrideOf(inst, pix);
}
// Frames per pipeline step of pairs_kernel.
constexpr uint32_t kPairsGroup = 4;
// The decoded band in LDS: per frame of a group, 8 rows of the piece (9 with the row below: row 0 of the next tile
// row), each 64 dwords of pixels between two guard dwords on either side, padded to 72 so that a half wave's 8-byte
// accesses fall into 64 different banks.  Double-buffered: one barrier per group.
constexpr uint32_t kPairsRowDwords = 72;
constexpr uint32_t kPairsBandRowsOf(uint32_t inst) { return (inst & ~kPairRight) ? 9u : 8u; }
// LDS of one pairs_kernel workgroup: the band, the double-buffered wave totals of a group (for the piece and for the
// row below) and write_count's wave counts.
constexpr uint32_t kPairsLdsBytesOf(uint32_t inst) {
    return 2u * kPairsGroup * kPairsBandRowsOf(inst) * kPairsRowDwords * 4u +
           2u * kPairsGroup * (kPairsBandRowsOf(inst) - 7u) * 2u * (kProjThreads / 64u) * 4u + (kProjThreads / 64u) * 4u;
}

struct PairsParams {
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
    uint32_t rows, pieces;          // window tile rows; workgroups across one (kPairsPiecesOf)
    uint32_t segments, fps;         // frame segments; frames per segment (the last may hold fewer)
    int accumulate;                 // 1: add this call's sums to what the planes hold
    uint32_t pairs;                 // requested offsets, 1..15; plane j is the j-th set bit
    uint32_t planes;                // popcount(pairs)
    uint64_t *out;                  // [planes][rh][rw]
    uint64_t *out_count;
    void *ws;                       // per-segment partials [segments][planes][rh * rw], U32 (pix 1) or U64 (pix 2)
};

// pairs_kernel<kPairsInstanceOf(p.pairs), pix> (pix: 1 = DBDE, 2 = DBDE16): grid = pieces * rows * segments workgroups
// of kProjThreads; with segments > 1 pairs_combine_kernel follows on the same stream.
hipError_t launch_pairs(const PairsParams &p, uint32_t pix, hipStream_t s);
// Bytes of the per-segment partials of a window of `pixels` pixels: (4 * pix) * segments * planes * pixels rounded up
// to 16 (0 for one segment).
uint64_t pairs_workspace_bytes(uint32_t planes, uint32_t segments, uint64_t pixels, uint32_t pix);

}  // namespace dbde
