// dbde_scaled_kernels.h -- launch interface of the scaled float decode (dbde_hip_decode_scaled), dbde_scaled_kernels.hip.
//
// A scaled decode writes the rw x rh window of each frame as floating point: v = ((float)p - D) * G per pixel, D and G
// from F32 maps in frame coordinates or scalars, rounded once to F32 / F16 / BF16.  Validation and the per-chunk payload
// offsets come from the decode index kernel run with the window decoder's chunk geometry (roi_index_geometry), exactly
// as dbde_hip_decode_roi runs it; decode_scaled_kernel has decode_roi_kernel's steps 1-3 (one tile per thread, its
// payload cut out of LDS into a band of pixels) and converts the band on its way out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_roi_kernels.h"

namespace dbde {

// Output types: the values of DBDE_HIP_OUT_F32 / _F16 / _BF16 (include/dbde_hip.h).
constexpr uint32_t kScaledF32 = 0, kScaledF16 = 1, kScaledBF16 = 2;
constexpr uint32_t kScaledElemBytesOf(uint32_t out) { return out == kScaledF32 ? 4u : 2u; }

// Tiles of one window tile row that one workgroup takes (one tile per thread): the window decoder's piece widths.
constexpr uint32_t kScaledNarrowThreads = kRoiNarrowThreads;   // windows of at most 64 tiles across
constexpr uint32_t kScaledWideThreadsOf(uint32_t pix) { return pix == 1u ? kRoiWideThreads : kRoi16WideThreads; }
// LDS per workgroup: the piece's payload (threads tiles of depth 8 * pix, the aligned head and the cutter's over-read),
// reused as the band of 8 image rows in the pixel type, and the block scan's 2 x waves words.
constexpr uint32_t kScaledPayBytesOf(uint32_t threads, uint32_t pix) { return pix == 1u ? threads * 64u + 64u : threads * 128u + 32u; }
constexpr uint32_t kScaledLdsBytesOf(uint32_t threads, uint32_t pix) { return kScaledPayBytesOf(threads, pix) + 8u * (threads / 64u); }

struct ScaledParams {
    RoiParams roi;        // the window decoder's parameters; roi.out is the output (F32 / F16 / BF16 elements)
    const float *dark;    // optional [H][W] map in frame coordinates; NULL -> dark0
    const float *gain;    // optional [H][W] map in frame coordinates; NULL -> gain0
    float dark0, gain0;
};

// One workgroup per (frame, window tile row, piece of `threads` tiles); grid = n_frames * roi.rows * roi.pieces.  pix:
// bytes per pixel, 1 = DBDE, 2 = DBDE16; threads: kScaledNarrowThreads or kScaledWideThreadsOf(pix); out: kScaledF32,
// kScaledF16 or kScaledBF16.
hipError_t launch_decode_scaled(const ScaledParams &p, uint32_t n_frames, uint32_t threads, uint32_t pix, uint32_t out,
                                hipStream_t s);

}  // namespace dbde
