// dbde_roi_kernels.hip -- window (region-of-interest) decode for MI355X (gfx950, wave64).
//
// Decodes the rw x rh window of each frame without touching the rest of the frame's payload.  Tiles are independent and
// a tile's payload starts at the prefix sum of the depth bytes in front of it, so a window needs only
//   * the depth array (all of it, once per frame, for the validation: decode_index_kernel in dbde_kernels.hip, run with
//     chunks that start at every tile row -- roi_index_geometry);
//   * the depth and minimum bytes of the window's tiles, plus fewer than 512 depth bytes in front of each window tile
//     row's first tile (from its chunk's start);
//   * the payload of the window's tiles, one contiguous byte range per window tile row;
//   * the window's output.
//
// decode_roi_kernel<THREADS, PIX>: PIX = 1 for DBDE frames (U8 pixels and minima, depth 0..8, payload at 32 + 2T), PIX = 2
// for DBDE16 frames (U16 pixels and minima, depth 0..16, payload at 32 + 3T).  One workgroup per (frame, window tile row,
// piece of THREADS tiles), one tile per thread:
//   1. the tiles' depth / minimum bytes (a U16 minimum is read byte by byte: the array starts at 28 + T, so it can sit
//      at an odd address) and the depth bytes in front of the piece; one block scan gives each tile's payload word
//      offset inside the piece and the piece's offset inside the frame;
//   2. the piece's payload range, fetched as 16-byte blocks from the aligned address in front of it into LDS (the block
//      that would cross stream_bytes byte by byte);
//   3. each thread cuts its tile's 8 rows out of LDS into registers, then into an LDS band of 8 image rows that reuses
//      the payload buffer.  A row is 8d bits at byte r*d of the tile.  PIX = 1: three aligned dwords and v_alignbyte per
//      row, dbde_bits.h's expand_row / add_bytes.  PIX = 2: dbde_device.h's cut_row16, dec16_kernel's cut;
//   4. the window's part of the band leaves as ONE contiguous output range when the piece spans the whole window width
//      (up to 8 rw pixels), row by row otherwise: aligned 16-byte stores, single pixels only at the range's two ends.
// Latency is hidden by occupancy (each workgroup is short: one dependent global load chain), not by a software pipeline.
#include "dbde_roi_kernels.h"

#include <type_traits>

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));   // native vector for the nontemporal builtins

}  // namespace

template <uint32_t THREADS, uint32_t PIX>
__global__ __launch_bounds__(THREADS) void decode_roi_kernel(RoiParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    typedef typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type Pix;
    typedef typename std::conditional<PIX == 1u, uint2, uint4>::type Row;   // one tile row of 8 pixels
    constexpr uint32_t NW = THREADS / 64u;
    // THREADS tiles of depth 8 * PIX, the aligned head (and tail), the cutter's over-read
    constexpr uint32_t kPayBytes = PIX == 1u ? THREADS * 64u + 64u : THREADS * 128u + 32u;
    constexpr uint32_t kPitch = THREADS * 8u;   // band row in pixels: THREADS tiles of 8 pixels
    // one buffer: the payload, then (once every tile is cut into registers) the band -- half the LDS, twice the
    // workgroups per CU of two separate arrays (8-bit full-frame windows: 9 instead of 4)
    __shared__ __attribute__((aligned(16))) uint32_t s_pay[kPayBytes / 4u];
    static_assert(8u * PIX * kPitch + 4u <= kPayBytes, "the band must fit the payload buffer");
    const Pix *band = reinterpret_cast<const Pix *>(s_pay);
    __shared__ uint32_t s_wsum[2][NW];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per_frame = p.rows * p.pieces;
    const uint32_t f = blockIdx.x / per_frame;
    const uint32_t rem = blockIdx.x - f * per_frame;
    const uint32_t br = rem / p.pieces, pc = rem - br * p.pieces;
    if (!p.frame_ok[f]) return;   // rejected frame: its window stays untouched

    int x = p.x0, y = p.y0;
    if (p.origins) {   // a tracker's moving window, clamped into the frame
        x = p.origins[2u * f];
        y = p.origins[2u * f + 1u];
        x = x < 0 ? 0 : (x > p.W - p.rw ? p.W - p.rw : x);
        y = y < 0 ? 0 : (y > p.H - p.rh ? p.H - p.rh : y);
    }
    const uint32_t tx_a = (uint32_t)x >> 3, tx_b = (uint32_t)(x + p.rw - 1) >> 3;
    const uint32_t ty_a = (uint32_t)y >> 3, ty_b = (uint32_t)(y + p.rh - 1) >> 3;
    const uint32_t ty = ty_a + br, txp = tx_a + pc * THREADS;
    if (ty > ty_b || txp > tx_b) return;   // the grid covers the most any origin needs
    const uint32_t nt = tx_b + 1u - txp < THREADS ? tx_b + 1u - txp : THREADS;

    // ---- 1. depth / minimum bytes, offsets ----
    const uint8_t *fb = p.stream + p.frame_offsets[f];   // validated: the whole frame lies inside stream_bytes
    const uint8_t *darr = fb + 24;
    const uint8_t *marr = fb + 28 + p.T;
    const uint8_t *pay = fb + 32 + (PIX + 1ull) * p.T;
    const uint32_t pos0 = ty * p.w + txp;
    const uint32_t c = dec_chunk_of(p.geom, pos0), cb = dec_chunk_begin(p.geom, c);
    const uint32_t base = p.chunk_off[(size_t)f * (p.geom.cpf + 1u) + c];
    const uint32_t npre = pos0 - cb;   // < 512 (roi_index_geometry)
    uint32_t pre = 0;
#pragma unroll
    for (uint32_t k = 0; k < kChunkTiles / THREADS; k++) {
        const uint32_t j = tid + k * THREADS;
        if (j < npre) pre += darr[cb + j];
    }
    uint32_t d = 0, mn = 0;
    if (tid < nt) {
        d = darr[pos0 + tid];
        if constexpr (PIX == 1u) {
            mn = marr[pos0 + tid];
        } else {
            const uint8_t *m = marr + 2u * (pos0 + tid);
            mn = (uint32_t)m[0] | ((uint32_t)m[1] << 8);
        }
    }
    d = d > 8u * PIX ? 8u * PIX : d;   // (a validated frame has none)
    const uint32_t incl = wave_scan_incl(d);
    const uint32_t pre_w = wave_sum(pre);
    if (lane == 63u) s_wsum[0][wave] = incl;
    if (lane == 0u) s_wsum[1][wave] = pre_w;
    __syncthreads();
    uint32_t wbase = 0, S = 0, PRE = 0;
#pragma unroll
    for (uint32_t k = 0; k < NW; k++) {
        const uint32_t v = s_wsum[0][k];
        wbase += k < wave ? v : 0u;
        S += v;
        PRE += s_wsum[1][k];
    }
    const uint32_t woff = wbase + incl - d;   // payload words in front of this tile inside the piece

    // ---- 2. the piece's payload into LDS ----
    const uint8_t *src0 = pay + 8ull * ((uint64_t)base + PRE);
    const uint8_t *a_lo = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(src0) & ~(uintptr_t)15);
    const uint32_t sh = (uint32_t)(src0 - a_lo);
    const uint32_t nblk = (sh + 8u * S + 15u) >> 4;   // <= 4 * PIX * THREADS + 1
    const uint8_t *end = p.stream + p.stream_bytes;
    for (uint32_t i = tid; i < nblk; i += THREADS) {
        const uint8_t *q = a_lo + 16u * i;
        uint4 v;
        if (q + 16 <= end) {
            const u32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(q));   // streamed once
            v = make_uint4(t.x, t.y, t.z, t.w);
        } else {   // the block that crosses the readable extent: only the bytes in front of it
            uint32_t wq[4] = {0, 0, 0, 0};
            for (uint32_t b = 0; b < 16u; b++)
                if (q + b < end) wq[b >> 2] |= (uint32_t)q[b] << (8u * (b & 3u));
            v = make_uint4(wq[0], wq[1], wq[2], wq[3]);
        }
        *reinterpret_cast<uint4 *>(s_pay + 4u * i) = v;
    }
    __syncthreads();

    // ---- 3. tile rows -> registers -> the band ----
    Row px[8];
    if (tid < nt) {
        if constexpr (PIX == 1u) {
            const uint32_t mm = mn * 0x01010101u;
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                const uint32_t o = sh + 8u * woff + r * d;   // byte of tile row r (8d bits)
                const uint32_t w0 = o >> 2, s = o & 3u;
                const uint32_t a0 = s_pay[w0], a1 = s_pay[w0 + 1u], a2 = s_pay[w0 + 2u];
                const uint64_t bits = (uint64_t)__builtin_amdgcn_alignbyte(a1, a0, s) |
                                      ((uint64_t)__builtin_amdgcn_alignbyte(a2, a1, s) << 32);
                uint32_t lo, hi;
                expand_row(bits, d, lo, hi);
                px[r] = make_uint2(add_bytes(lo, mm), add_bytes(hi, mm));
            }
        } else {
            const uint32_t byte0 = sh + 8u * woff;
            const uint32_t m32 = d >= 16u ? 0xFFFFu : (1u << d) - 1u, mn2 = mn * 0x00010001u;
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                const uint32_t a = byte0 + r * d, ah = a + (d >> 1);   // the row's two 4-pixel halves
                cut_row16(s_pay + (a >> 2), s_pay + (ah >> 2), a, ah, d, m32, mn2, px[r].x, px[r].y, px[r].z, px[r].w);
            }
        }
    }
    __syncthreads();   // every tile cut: the payload buffer becomes the band
    if (tid < nt) {
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++)
            *reinterpret_cast<Row *>(reinterpret_cast<uint8_t *>(s_pay) + PIX * (r * kPitch + 8u * tid)) = px[r];
    }
    __syncthreads();

    // ---- 4. the window's part of the band -> the output (in pixels) ----
    constexpr uint32_t kPerDword = 4u / PIX, kPerBlock = 16u / PIX;
    const int px0 = 8 * (int)txp;                                       // first pixel column of the piece
    const int c_lo = px0 > x ? px0 : x;
    const int c_hi = px0 + 8 * (int)nt < x + p.rw ? px0 + 8 * (int)nt : x + p.rw;
    const int r_lo = 8 * (int)ty > y ? 8 * (int)ty : y;
    const int r_hi = 8 * (int)ty + 8 < y + p.rh ? 8 * (int)ty + 8 : y + p.rh;
    const uint32_t pw = (uint32_t)(c_hi - c_lo), nr = (uint32_t)(r_hi - r_lo);
    const uint32_t bx = (uint32_t)(c_lo - px0), by = (uint32_t)(r_lo - 8 * (int)ty);
    Pix *dst = reinterpret_cast<Pix *>(p.out) + (size_t)f * (size_t)p.rw * (size_t)p.rh + (size_t)(r_lo - y) * (size_t)p.rw +
               (size_t)(c_lo - x);
    const bool whole = pw == (uint32_t)p.rw;   // rows of the window are adjacent in the output: one range
    const uint32_t nseg = whole ? 1u : nr, len = whole ? nr * pw : pw;
    for (uint32_t sg = 0; sg < nseg; sg++) {
        Pix *g = dst + (size_t)sg * (size_t)p.rw;
        const uintptr_t g0 = reinterpret_cast<uintptr_t>(g), a0 = g0 & ~(uintptr_t)15, g1 = g0 + PIX * len;
        const uint32_t nb = (uint32_t)((g1 - a0 + 15u) >> 4);
        for (uint32_t i = tid; i < nb; i += THREADS) {
            const uintptr_t ba = a0 + 16u * i;
            const uint32_t lo = ba < g0 ? (uint32_t)(g0 - ba) / PIX : 0u;        // pixels of the block inside the range
            const uint32_t hi = ba + 16u > g1 ? (uint32_t)(g1 - ba) / PIX : kPerBlock;
            const uint32_t L = sg * len + (uint32_t)(ba + PIX * lo - g0) / PIX;   // (row, column) of the first pixel, row-major at pitch pw
            uint32_t row = L / pw, col = L - row * pw;
            if (lo == 0u && hi == kPerBlock) {
                uint32_t v[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (col + kPerDword <= pw) {
                        v[k] = lds_u32_at(s_pay, PIX * ((by + row) * kPitch + bx + col));
                        col += kPerDword;
                        if (col == pw) { col = 0; row++; }
                    } else {   // a window row ends inside the dword
                        uint32_t t = 0;
                        for (uint32_t b = 0; b < kPerDword; b++) {
                            t |= (uint32_t)band[(by + row) * kPitch + bx + col] << (8u * PIX * b);
                            if (++col == pw) { col = 0; row++; }
                        }
                        v[k] = t;
                    }
                }
                u32x4_t o;
                o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
                __builtin_nontemporal_store(o, reinterpret_cast<u32x4_t *>(ba));   // the window is written once
            } else {   // the range's first / last block: the pixels inside it only
                for (uint32_t b = lo; b < hi; b++) {
                    reinterpret_cast<Pix *>(ba)[b] = band[(by + row) * kPitch + bx + col];
                    if (++col == pw) { col = 0; row++; }
                }
            }
        }
    }
}

hipError_t launch_decode_roi(const RoiParams &p, uint32_t n_frames, uint32_t threads, uint32_t pix, hipStream_t s) {
    const uint32_t grid = n_frames * p.rows * p.pieces;   // (the host keeps it below 2^31)
    if (pix == 1u) {
        if (threads == kRoiNarrowThreads)
            hipLaunchKernelGGL((decode_roi_kernel<kRoiNarrowThreads, 1>), dim3(grid), dim3(kRoiNarrowThreads), 0, s, p);
        else
            hipLaunchKernelGGL((decode_roi_kernel<kRoiWideThreads, 1>), dim3(grid), dim3(kRoiWideThreads), 0, s, p);
    } else {
        if (threads == kRoiNarrowThreads)
            hipLaunchKernelGGL((decode_roi_kernel<kRoiNarrowThreads, 2>), dim3(grid), dim3(kRoiNarrowThreads), 0, s, p);
        else
            hipLaunchKernelGGL((decode_roi_kernel<kRoi16WideThreads, 2>), dim3(grid), dim3(kRoi16WideThreads), 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace dbde
