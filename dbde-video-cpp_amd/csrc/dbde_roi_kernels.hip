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
// decode_roi_kernel: one workgroup per (frame, window tile row, piece of THREADS tiles), one tile per thread:
//   1. the tiles' depth / minimum bytes and the depth bytes in front of the piece; one block scan gives each tile's
//      payload word offset inside the piece and the piece's offset inside the frame;
//   2. the piece's payload range, fetched as 16-byte blocks from the aligned address in front of it into LDS (the block
//      that would cross stream_bytes byte by byte);
//   3. each thread cuts its tile's 8 rows out of LDS (three aligned dwords and v_alignbyte per row, dbde_bits.h's
//      expand_row / add_bytes) into registers, then into an LDS band of 8 image rows that reuses the payload buffer;
//   4. the window's part of the band leaves as ONE contiguous output range when the piece spans the whole window width
//      (up to 8 rw bytes), row by row otherwise: aligned 16-byte stores, bytes only at the range's two ends.
// Latency is hidden by occupancy (each workgroup is short: one dependent global load chain), not by a software pipeline.
// decode_roi16_kernel (below) is the same for DBDE16 frames: U16 minima and pixels, depth 0..16.
#include "dbde_roi_kernels.h"

#include "dbde_bits.h"

namespace dbde {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));   // native vector for the nontemporal builtins

__device__ __forceinline__ uint32_t roi_wave_scan_incl(uint32_t x) {   // DPP row shifts / broadcasts, no LDS
    uint32_t t = x;
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x111, 0xF, 0xF, false);   // row_shr:1
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x112, 0xF, 0xF, false);   // row_shr:2
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x114, 0xF, 0xF, false);   // row_shr:4
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x118, 0xF, 0xF, false);   // row_shr:8
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1,3
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2,3
    return t;
}

__device__ __forceinline__ uint32_t roi_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The four bytes at LDS byte address a (any alignment; the dword after the one holding a must be inside the array).
__device__ __forceinline__ uint32_t lds_u32_at(const uint32_t *s32, uint32_t a) {
    return __builtin_amdgcn_alignbyte(s32[(a >> 2) + 1u], s32[a >> 2], a & 3u);
}

}  // namespace

template <uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void decode_roi_kernel(RoiParams p) {
    constexpr uint32_t NW = THREADS / 64u;
    constexpr uint32_t kPayBytes = THREADS * 64u + 64u;   // THREADS tiles of depth 8, the aligned head and tail, the cutter's over-read
    constexpr uint32_t kPitch = THREADS * 8u;             // band row: THREADS tiles of 8 pixels
    // one buffer: the payload, then (once every tile is cut into registers) the band -- half the LDS, twice the
    // workgroups per CU of two separate arrays (full-frame windows: 9 instead of 4)
    __shared__ __attribute__((aligned(16))) uint32_t s_pay[kPayBytes / 4u];
    static_assert(8u * kPitch + 16u <= kPayBytes, "the band must fit the payload buffer");
    uint32_t *s_band = s_pay;
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
    const uint8_t *pay = fb + 32 + 2ull * p.T;
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
        mn = marr[pos0 + tid];
    }
    d = d > 8u ? 8u : d;   // (a validated frame has none)
    const uint32_t incl = roi_wave_scan_incl(d);
    const uint32_t pre_w = roi_wave_sum(pre);
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
    const uint32_t nblk = (sh + 8u * S + 15u) >> 4;   // <= 4 * THREADS + 1
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
    uint2 px[8];
    if (tid < nt) {
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
    }
    __syncthreads();   // every tile cut: the payload buffer becomes the band
    if (tid < nt) {
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++)
            *reinterpret_cast<uint2 *>(reinterpret_cast<uint8_t *>(s_band) + r * kPitch + 8u * tid) = px[r];
    }
    __syncthreads();

    // ---- 4. the window's part of the band -> the output ----
    const int px0 = 8 * (int)txp;                                       // first pixel column of the piece
    const int c_lo = px0 > x ? px0 : x;
    const int c_hi = px0 + 8 * (int)nt < x + p.rw ? px0 + 8 * (int)nt : x + p.rw;
    const int r_lo = 8 * (int)ty > y ? 8 * (int)ty : y;
    const int r_hi = 8 * (int)ty + 8 < y + p.rh ? 8 * (int)ty + 8 : y + p.rh;
    const uint32_t pw = (uint32_t)(c_hi - c_lo), nr = (uint32_t)(r_hi - r_lo);
    const uint32_t bx = (uint32_t)(c_lo - px0), by = (uint32_t)(r_lo - 8 * (int)ty);
    const uint8_t *band = reinterpret_cast<const uint8_t *>(s_band);
    uint8_t *dst = p.out + (size_t)f * (size_t)p.rw * (size_t)p.rh + (size_t)(r_lo - y) * (size_t)p.rw + (size_t)(c_lo - x);
    const bool whole = pw == (uint32_t)p.rw;   // rows of the window are adjacent in the output: one range
    const uint32_t nseg = whole ? 1u : nr, len = whole ? nr * pw : pw;
    for (uint32_t sg = 0; sg < nseg; sg++) {
        uint8_t *g = dst + (size_t)sg * (size_t)p.rw;
        const uintptr_t g0 = reinterpret_cast<uintptr_t>(g), a0 = g0 & ~(uintptr_t)15;
        const uint32_t nb = (uint32_t)((g0 + len - a0 + 15u) >> 4);
        for (uint32_t i = tid; i < nb; i += THREADS) {
            const uintptr_t ba = a0 + 16u * i;
            const uint32_t lo = ba < g0 ? (uint32_t)(g0 - ba) : 0u;
            const uint32_t hi = ba + 16u > g0 + len ? (uint32_t)(g0 + len - ba) : 16u;
            const uint32_t L = sg * len + (uint32_t)(ba + lo - g0);   // (row, column) of the first byte, row-major at pitch pw
            uint32_t row = L / pw, col = L - row * pw;
            if (lo == 0u && hi == 16u) {
                uint32_t v[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (col + 4u <= pw) {
                        v[k] = lds_u32_at(s_band, (by + row) * kPitch + bx + col);
                        col += 4u;
                        if (col == pw) { col = 0; row++; }
                    } else {
                        uint32_t t = 0;
                        for (uint32_t b = 0; b < 4u; b++) {
                            t |= (uint32_t)band[(by + row) * kPitch + bx + col] << (8u * b);
                            if (++col == pw) { col = 0; row++; }
                        }
                        v[k] = t;
                    }
                }
                u32x4_t o;
                o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
                __builtin_nontemporal_store(o, reinterpret_cast<u32x4_t *>(ba));   // the window is written once
            } else {   // the range's first / last block: the bytes inside it only
                for (uint32_t b = lo; b < hi; b++) {
                    reinterpret_cast<uint8_t *>(ba)[b] = band[(by + row) * kPitch + bx + col];
                    if (++col == pw) { col = 0; row++; }
                }
            }
        }
    }
}

// decode_roi16_kernel: DBDE16 windows (U16 pixels, depth 0..16, U16 minima at 28 + T from the frame data, payload at
// 32 + 3T), decode_roi_kernel's shape with U16 tiles:
//   1. the tiles' depth bytes and minima (two bytes each: the array starts at 28 + T, so a minimum can sit at an odd
//      address) and the depth bytes in front of the piece; one DPP scan as above;
//   2. the piece's payload range into LDS as above (up to 128 bytes per tile);
//   3. each tile row is 8d bits at byte r*d of the tile: its two 4-pixel halves come out of three aligned dwords each
//      (v_alignbyte; the second half starts d/2 bytes, plus 4 bits when d is odd, later), a pixel is one v_alignbit at
//      i*d, the minimum is added modulo 2^16 with v_pk_add_u16 -- dec16_kernel's cut; into registers, then into an LDS
//      band of 8 image rows of 16 bytes per tile that reuses the payload buffer;
//   4. the window's part of the band leaves as in decode_roi_kernel, in U16 pixels: aligned 16-byte stores, single
//      pixels only at the two ends of each contiguous range (the output is 2-byte aligned).
template <uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void decode_roi16_kernel(RoiParams p) {
    constexpr uint32_t NW = THREADS / 64u;
    constexpr uint32_t kPayBytes = THREADS * 128u + 32u;   // THREADS tiles of depth 16, the aligned head, the cutter's over-read
    constexpr uint32_t kPitch = THREADS * 8u;              // band row in pixels: THREADS tiles of 8 pixels
    // one buffer, as in decode_roi_kernel: the payload, then (once every tile is cut into registers) the band
    __shared__ __attribute__((aligned(16))) uint32_t s_pay[kPayBytes / 4u];
    static_assert(16u * kPitch + 4u <= kPayBytes, "the band must fit the payload buffer");
    const uint16_t *band = reinterpret_cast<const uint16_t *>(s_pay);
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

    // ---- 1. depth bytes / minima, offsets ----
    const uint8_t *fb = p.stream + p.frame_offsets[f];   // validated: the whole frame lies inside stream_bytes
    const uint8_t *darr = fb + 24;
    const uint8_t *marr = fb + 28 + p.T;
    const uint8_t *pay = fb + 32 + 3ull * p.T;
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
        const uint8_t *m = marr + 2u * (pos0 + tid);
        mn = (uint32_t)m[0] | ((uint32_t)m[1] << 8);
    }
    d = d > 16u ? 16u : d;   // (a validated frame has none)
    const uint32_t incl = roi_wave_scan_incl(d);
    const uint32_t pre_w = roi_wave_sum(pre);
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
    const uint32_t nblk = (sh + 8u * S + 15u) >> 4;   // <= 8 * THREADS + 1
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
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    uint4 px[8];
    if (tid < nt) {
        const uint32_t byte0 = sh + 8u * woff;
        const uint32_t m32 = d >= 16u ? 0xFFFFu : (1u << d) - 1u, mn2 = mn * 0x00010001u, sh_odd = (d & 1u) * 4u;
        const bool c2 = 2u * d >= 32u, c3 = 3u * d >= 32u;
        // four pixels of d bits at bit 0 of the 64-bit window x1:x0 (shift counts modulo 32: from bit 32 on, x1 is shifted)
        auto four = [&](uint32_t x0, uint32_t x1, uint32_t &o0, uint32_t &o1) __attribute__((always_inline)) {
            const uint32_t p0 = x0 & m32;
            const uint32_t p1 = __builtin_amdgcn_alignbit(x1, x0, d) & m32;
            const uint32_t p2 = __builtin_amdgcn_alignbit(c2 ? 0u : x1, c2 ? x1 : x0, 2u * d) & m32;
            const uint32_t p3 = __builtin_amdgcn_alignbit(c3 ? 0u : x1, c3 ? x1 : x0, 3u * d) & m32;
            o0 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, p0 | (p1 << 16)) + __builtin_bit_cast(u16x2, mn2));
            o1 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, p2 | (p3 << 16)) + __builtin_bit_cast(u16x2, mn2));
        };
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++) {
            const uint32_t a = byte0 + r * d, ah = a + (d >> 1);   // the row's two 4-pixel halves
            const uint32_t *q = s_pay + (a >> 2), *qh = s_pay + (ah >> 2);
            const uint32_t x0 = __builtin_amdgcn_alignbyte(q[1], q[0], a), x1 = __builtin_amdgcn_alignbyte(q[2], q[1], a);
            const uint32_t w0 = __builtin_amdgcn_alignbyte(qh[1], qh[0], ah), w1 = __builtin_amdgcn_alignbyte(qh[2], qh[1], ah);
            const uint32_t h0 = __builtin_amdgcn_alignbit(w1, w0, sh_odd), h1 = w1 >> sh_odd;
            four(x0, x1, px[r].x, px[r].y);
            four(h0, h1, px[r].z, px[r].w);
        }
    }
    __syncthreads();   // every tile cut: the payload buffer becomes the band
    if (tid < nt) {
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++) *reinterpret_cast<uint4 *>(s_pay + 4u * (r * (kPitch / 8u) + tid)) = px[r];
    }
    __syncthreads();

    // ---- 4. the window's part of the band -> the output (in pixels) ----
    const int px0 = 8 * (int)txp;                                       // first pixel column of the piece
    const int c_lo = px0 > x ? px0 : x;
    const int c_hi = px0 + 8 * (int)nt < x + p.rw ? px0 + 8 * (int)nt : x + p.rw;
    const int r_lo = 8 * (int)ty > y ? 8 * (int)ty : y;
    const int r_hi = 8 * (int)ty + 8 < y + p.rh ? 8 * (int)ty + 8 : y + p.rh;
    const uint32_t pw = (uint32_t)(c_hi - c_lo), nr = (uint32_t)(r_hi - r_lo);
    const uint32_t bx = (uint32_t)(c_lo - px0), by = (uint32_t)(r_lo - 8 * (int)ty);
    uint16_t *dst = reinterpret_cast<uint16_t *>(p.out) + (size_t)f * (size_t)p.rw * (size_t)p.rh +
                    (size_t)(r_lo - y) * (size_t)p.rw + (size_t)(c_lo - x);
    const bool whole = pw == (uint32_t)p.rw;   // rows of the window are adjacent in the output: one range
    const uint32_t nseg = whole ? 1u : nr, len = whole ? nr * pw : pw;
    for (uint32_t sg = 0; sg < nseg; sg++) {
        uint16_t *g = dst + (size_t)sg * (size_t)p.rw;
        const uintptr_t g0 = reinterpret_cast<uintptr_t>(g), a0 = g0 & ~(uintptr_t)15, g1 = g0 + 2u * len;
        const uint32_t nb = (uint32_t)((g1 - a0 + 15u) >> 4);
        for (uint32_t i = tid; i < nb; i += THREADS) {
            const uintptr_t ba = a0 + 16u * i;
            const uint32_t lo = ba < g0 ? (uint32_t)(g0 - ba) >> 1 : 0u;        // pixels of the block inside the range
            const uint32_t hi = ba + 16u > g1 ? (uint32_t)(g1 - ba) >> 1 : 8u;
            const uint32_t L = sg * len + ((uint32_t)(ba + 2u * lo - g0) >> 1);   // (row, column) of the first pixel, row-major at pitch pw
            uint32_t row = L / pw, col = L - row * pw;
            if (lo == 0u && hi == 8u) {
                uint32_t v[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (col + 2u <= pw) {
                        v[k] = lds_u32_at(s_pay, 2u * ((by + row) * kPitch + bx + col));
                        col += 2u;
                        if (col == pw) { col = 0; row++; }
                    } else {   // a window row ends inside the dword
                        uint32_t t = band[(by + row) * kPitch + bx + col];
                        if (++col == pw) { col = 0; row++; }
                        t |= (uint32_t)band[(by + row) * kPitch + bx + col] << 16;
                        if (++col == pw) { col = 0; row++; }
                        v[k] = t;
                    }
                }
                u32x4_t o;
                o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
                __builtin_nontemporal_store(o, reinterpret_cast<u32x4_t *>(ba));   // the window is written once
            } else {   // the range's first / last block: the pixels inside it only
                for (uint32_t b = lo; b < hi; b++) {
                    reinterpret_cast<uint16_t *>(ba)[b] = band[(by + row) * kPitch + bx + col];
                    if (++col == pw) { col = 0; row++; }
                }
            }
        }
    }
}

hipError_t launch_decode_roi(const RoiParams &p, uint32_t n_frames, uint32_t threads, hipStream_t s) {
    const uint32_t grid = n_frames * p.rows * p.pieces;   // (the host keeps it below 2^31)
    if (threads == kRoiNarrowThreads)
        hipLaunchKernelGGL(decode_roi_kernel<kRoiNarrowThreads>, dim3(grid), dim3(kRoiNarrowThreads), 0, s, p);
    else
        hipLaunchKernelGGL(decode_roi_kernel<kRoiWideThreads>, dim3(grid), dim3(kRoiWideThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_decode_roi16(const RoiParams &p, uint32_t n_frames, uint32_t threads, hipStream_t s) {
    const uint32_t grid = n_frames * p.rows * p.pieces;   // (the host keeps it below 2^31)
    if (threads == kRoiNarrowThreads)
        hipLaunchKernelGGL(decode_roi16_kernel<kRoiNarrowThreads>, dim3(grid), dim3(kRoiNarrowThreads), 0, s, p);
    else
        hipLaunchKernelGGL(decode_roi16_kernel<kRoi16WideThreads>, dim3(grid), dim3(kRoi16WideThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
