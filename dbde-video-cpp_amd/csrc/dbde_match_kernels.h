// dbde_match_kernels.h -- launch interface of the patch match, dbde_match_kernels.hip.
//
// The patch match reuses the decode index kernel on the window decoder's chunk geometry (roi_index_geometry: one index
// pass serves any number of patches) and adds one kernel, templated on the pixel size, that decodes a search patch of
// (tw + 2S) x (th + 2S) pixels into LDS and reduces it against a tw x th template at each of the (2S + 1)^2 shifts: the
// exact sums of T P, of P and of P^2 under the template, one 256-lane workgroup per (frame, patch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_roi_kernels.h"

namespace dbde {

constexpr uint32_t kMatchThreads = 256;    // four waves: up to four decode a group of tile rows each, all four reduce
constexpr uint32_t kMatchWaves = kMatchThreads / 64u;
constexpr int kMatchMaxTemplate = 128;     // tw, th: 128^2 * 255^2 < 2^32, an 8-bit entry fits a v_dot4_u32_u8 chain
constexpr int kMatchMaxRadius = 16;        // S: the search patch is at most 160 x 160, a surface at most 33 x 33
constexpr uint32_t kMatchMaxSlices = 16;   // row slices a shift is split into at most
constexpr uint32_t kMatchBatch = 4;        // dwords of a template row a lane reads at once
constexpr uint32_t kMatchItemCost = 3;     // an item's fixed cost in batches: two divisions, the LDS accumulation (listing)

constexpr uint32_t kMatchClamp = 0;   // the origin is clamped into the frame (the window decoder's rule)
constexpr uint32_t kMatchFill = 1;    // the patch sits where the origin says; pixels outside the frame are `fill`

constexpr uint32_t kMatchProd = 1, kMatchSum = 2, kMatchSq = 4;   // the surfaces (DBDE_HIP_MATCH_*)

// The LDS of one workgroup, sized per launch (PIX bytes per pixel), in bytes from the start of the dynamic LDS:
//   band  the decoded tiles the search patch can span, 8 * mty rows of 8 * mtx pixels at an ODD pitch in dwords (lanes
//         whose shifts differ in dy, or whose template rows differ, read rows apart: an odd pitch spreads them over the
//         banks), plus the re-aligning read's dword beyond the last row;
//   tmpl  the template, every row padded with zeros to whole dwords;
//   work  first the payload ranges of the decoding waves (G tile rows of mtx tiles each, as the patch decoder lays them
//         out), then, when a shift's rows are split over several lanes, the U64 accumulators of the three surfaces.
struct MatchLayout {
    uint32_t pitch;       // band row, dwords
    uint32_t tw4;         // template row, dwords
    uint32_t pay_wave;    // payload region of one decoding wave, bytes
    uint32_t off_tmpl, off_work;
    uint32_t bytes;       // the whole
};

// Bytes between the payload ranges of two tile rows of a wave (the patch decoder's).
__host__ __device__ constexpr uint32_t kMatchRowBytesOf(uint32_t mtx, uint32_t pix) { return 64u * pix * mtx + 32u; }

inline MatchLayout match_layout(uint32_t pix, uint32_t tw, uint32_t th, uint32_t S, uint32_t mtx, uint32_t mty, uint32_t G,
                                uint32_t dwaves, uint32_t slices) {
    MatchLayout l;
    const uint32_t D = 2u * S + 1u;
    l.pitch = (2u * mtx * pix) | 1u;
    l.tw4 = (tw * pix + 3u) / 4u;
    l.pay_wave = (G * kMatchRowBytesOf(mtx, pix) + 15u) & ~15u;
    const uint32_t band = (8u * mty * l.pitch * 4u + 16u + 15u) & ~15u;
    const uint32_t tmpl = (th * l.tw4 * 4u + 15u) & ~15u;
    const uint32_t pay = dwaves * l.pay_wave, acc = slices > 1u ? D * D * 24u : 0u;
    l.off_tmpl = band;
    l.off_work = band + tmpl;
    l.bytes = l.off_work + (pay > acc ? pay : acc);
    return l;
}

struct MatchParams {
    const uint8_t *stream;
    const uint64_t *frame_offsets;  // [n_frames]
    uint64_t stream_bytes;          // readable extent of stream
    const uint32_t *chunk_off;      // [n_frames][cpf + 1] from launch_decode_index
    const uint32_t *frame_ok;       // [n_frames]
    const int32_t *origins;         // [n_frames][n_patches][2] (x, y) of the search patch
    const uint32_t *counts;         // optional [n_frames]: live patches of the frame (clamped to n_patches)
    const uint8_t *templates;       // [n_templates][th][tw] pixels (U8; U16 for DBDE16 frames)
    uint64_t *prod, *sum, *sq;      // [n_frames][n_patches][D][D] each, NULL where not requested
    int32_t *used;                  // optional [n_frames][n_patches][2]: the origin used
    int W, H;
    int pw, ph;                     // the search patch: tw + 2S, th + 2S
    uint32_t tw, th, D;             // D = 2S + 1
    uint32_t n_patches;
    uint32_t per_patch;             // 1: template k belongs to patch k; 0: every patch uses template 0
    uint32_t w, h, T;
    DecGeom geom;                   // the index's chunk geometry (roi_index_geometry)
    uint32_t mtx;                   // the most tiles a search patch spans across
    uint32_t G;                     // tile rows per wave and step: max(1, 64 / mtx)
    uint32_t dwaves;                // decoding waves: min(4, groups of G tile rows)
    uint32_t steps;                 // steps of the decode loop: ceil(groups / dwaves)
    uint32_t slices;                // lanes that share a shift, each with every slices-th template row
    uint32_t mode;                  // kMatchClamp / kMatchFill
    uint32_t fill;                  // kMatchFill: the pixel outside the frame
    uint32_t stats;                 // kMatchProd | kMatchSum | kMatchSq
    MatchLayout lds;
    uint32_t block0;                // the workgroup number of this launch's first workgroup (launch_match_patches sets it)
};

// A launch's grid is counted in work-items: workgroups * kMatchThreads must stay below 2^32.
constexpr uint32_t kMatchMaxGrid = (1u << 24) - 1u;

// One workgroup per (frame, patch): n_frames * n_patches of them (the host keeps that below 2^31), in as many launches
// of at most kMatchMaxGrid workgroups as that takes.  pix: bytes per pixel, 1 = DBDE, 2 = DBDE16.
hipError_t launch_match_patches(const MatchParams &p, uint32_t n_frames, uint32_t pix, hipStream_t s);

}  // namespace dbde
