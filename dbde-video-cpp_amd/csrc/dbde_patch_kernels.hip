// dbde_patch_kernels.hip -- patch decode for MI355X (gfx950, wave64): K small windows of one size per frame.
//
// A tracker or a classifier wants a stack of small cut-outs per frame, one around each object.  The index pass
// (decode_index_kernel on roi_index_geometry's chunks) gives a payload offset at the start of every tile row, so it runs
// once per call however many patches there are; decode_patches_kernel<PIX> then decodes only the patches' tiles.
//
// decode_patches_kernel<PIX>: PIX = 1 for DBDE frames, PIX = 2 for DBDE16 frames.  One 64-lane workgroup per (frame,
// patch, group of G tile rows), one tile per lane: with mtx the most tiles a patch spans across, lane l takes tile
// (l / mtx, l % mtx) of the group, G = max(1, 64 / mtx).  A 32x32 patch (5 x 5 tiles) is one wave.  The steps are
// decode_roi_kernel's, made per tile row:
//   1. the tiles' depth / minimum bytes, and per tile row the fewer than 512 depth bytes between its chunk's start and
//      its first tile: the row's mtx lanes read them as aligned dwords with masked ends and sum them with v_sad_u8; one
//      wave scan, segmented per row, of (prefix bytes << 16 | depth) gives every row's payload start and every tile's
//      word offset inside its row;
//   2. each row's payload range (rows are separate contiguous stream ranges), fetched by the row's lanes as 16-byte
//      non-temporal blocks from the aligned address in front of it into the row's part of LDS (the block that would
//      cross stream_bytes byte by byte);
//   3. each lane cuts its tile's 8 rows out of LDS into registers (dbde_bits.h's expand_row / add_bytes, dbde_device.h's
//      cut_row16), then into an LDS band of 8 G image rows that reuses the payload buffer.  In fill mode a lane whose
//      tile lies outside the frame loads nothing and holds the fill pixel, and an edge tile's pixels beyond W or H are
//      replaced by it;
//   4. a patch is never wider than the workgroup, so the group's pixel rows of the patch are ONE contiguous output
//      range: aligned 16-byte non-temporal stores, single pixels only in the range's first and last block.
// Latency is hidden by occupancy, as in the window decoder.
#include "dbde_patch_kernels.h"

#include <type_traits>

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));   // native vector for the nontemporal builtins

constexpr uint32_t kPrefixBatch = 8;   // prefix dwords a lane has in flight at once

}  // namespace

template <uint32_t PIX>
__global__ __launch_bounds__(kPatchThreads) void decode_patches_kernel(PatchParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    typedef typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type Pix;
    typedef typename std::conditional<PIX == 1u, uint2, uint4>::type Row;   // one tile row of 8 pixels
    constexpr uint32_t kPayBytes = kPatchPayBytesOf(PIX);
    // one buffer: the rows' payload ranges, then (once every tile is cut into registers) the band
    __shared__ __attribute__((aligned(16))) uint32_t s_pay[kPayBytes / 4u];
    static_assert(kPatchThreads * 64u * PIX + 4u <= kPayBytes, "the band must fit the payload buffer");
    static_assert(kPatchThreads * 64u * PIX + 32u * kPatchThreads <= kPayBytes, "G <= 64 row ranges must fit");
    const Pix *band = reinterpret_cast<const Pix *>(s_pay);

    const uint32_t lane = threadIdx.x;
    uint32_t b = p.block0 + blockIdx.x;
    const uint32_t grp = b % p.groups;
    b /= p.groups;
    const uint32_t k = b % p.n_patches, f = b / p.n_patches;
    if (!p.frame_ok[f]) return;   // rejected frame: its patches stay untouched
    if (p.counts) {
        const uint32_t cnt = p.counts[f];
        if (k >= (cnt < p.n_patches ? cnt : p.n_patches)) return;   // not a live patch: untouched
    }
    const size_t pi = (size_t)f * p.n_patches + k;
    const int ox = p.origins[2u * pi], oy = p.origins[2u * pi + 1u];
    const bool fill_mode = p.mode == kPatchFill;
    int x, y;
    if (!fill_mode) {   // the window decoder's rule
        x = ox < 0 ? 0 : (ox > p.W - p.pw ? p.W - p.pw : ox);
        y = oy < 0 ? 0 : (oy > p.H - p.ph ? p.H - p.ph : oy);
    } else {   // any origin at or beyond these bounds gives the same patch, all fill
        x = ox < -p.pw ? -p.pw : (ox > p.W ? p.W : ox);
        y = oy < -p.ph ? -p.ph : (oy > p.H ? p.H : oy);
    }
    if (p.used && grp == 0u && lane == 0u) {
        p.used[2u * pi] = fill_mode ? ox : x;
        p.used[2u * pi + 1u] = fill_mode ? oy : y;
    }
    // tile coordinates are signed (a fill-mode patch can start left of or above the frame); ph has no limit: 64 bits
    const int64_t y_end = (int64_t)y + p.ph;
    const int tx_a = x >> 3, tx_b = (x + p.pw - 1) >> 3;
    const int64_t ty_a = y >> 3, ty_b = (y_end - 1) >> 3;
    const int64_t tyg = ty_a + (int64_t)grp * p.G;   // first tile row of the group
    if (tyg > ty_b) return;   // the grid covers the most any origin needs

    const uint32_t mtx = p.mtx;
    const uint32_t lr = lane / mtx, lc = lane - lr * mtx;
    const int64_t ty = tyg + lr;
    const int tx = tx_a + (int)lc;
    const bool row_live = lr < p.G && ty <= ty_b;
    const int txs = tx_a < 0 ? 0 : tx_a, txe = tx_b > (int)p.w - 1 ? (int)p.w - 1 : tx_b;
    const bool row_has = row_live && ty >= 0 && ty < (int64_t)p.h && txs <= txe;   // the row has tiles inside the frame
    const bool valid = row_has && tx >= txs && tx <= txe;

    // ---- 1. depth / minimum bytes, offsets ----
    const uint8_t *fb = p.stream + p.frame_offsets[f];   // validated: the whole frame lies inside stream_bytes
    const uint8_t *darr = fb + 24;
    const uint8_t *marr = fb + 28 + p.T;
    const uint8_t *pay = fb + 32 + (PIX + 1ull) * p.T;
    uint32_t base = 0, pre = 0;
    if (row_has) {
        const uint32_t pos0 = (uint32_t)ty * p.w + (uint32_t)txs;
        const uint32_t c = dec_chunk_of(p.geom, pos0), cb = dec_chunk_begin(p.geom, c);
        base = p.chunk_off[(size_t)f * (p.geom.cpf + 1u) + c];
        const uint32_t npre = pos0 - cb;   // < 512 (roi_index_geometry)
        if (npre) {
            // bytes [s, e) of the dwords at a0: the dwords lie inside the frame (24 header bytes in front, the row's own
            // depth bytes and the minima behind)
            const uintptr_t pa = reinterpret_cast<uintptr_t>(darr + cb);
            const uint32_t *a0 = reinterpret_cast<const uint32_t *>(pa & ~(uintptr_t)3);
            const uint32_t s = (uint32_t)(pa & 3u), e = s + npre, nd = (e + 3u) >> 2;   // nd <= 129
            for (uint32_t i0 = lc; i0 < nd; i0 += kPrefixBatch * mtx) {
                uint32_t v[kPrefixBatch];
#pragma unroll
                for (uint32_t j = 0; j < kPrefixBatch; j++) {   // (a clamped index keeps the loads unconditional: one batch)
                    const uint32_t i = i0 + j * mtx;
                    v[j] = a0[i < nd ? i : nd - 1u];
                }
#pragma unroll
                for (uint32_t j = 0; j < kPrefixBatch; j++) {
                    const uint32_t i = i0 + j * mtx;
                    uint32_t m = i < nd ? 0xFFFFFFFFu : 0u;
                    if (4u * i < s) m &= 0xFFFFFFFFu << (8u * (s - 4u * i));
                    if (4u * i + 4u > e) m &= 4u * i < e ? 0xFFFFFFFFu >> (8u * (4u * i + 4u - e)) : 0u;
                    pre = __builtin_amdgcn_sad_u8(v[j] & m, 0u, pre);
                }
            }
        }
    }
    uint32_t d = 0, mn = 0;
    if (valid) {
        const uint32_t pos = (uint32_t)ty * p.w + (uint32_t)tx;
        d = darr[pos];
        if constexpr (PIX == 1u) {
            mn = marr[pos];
        } else {
            const uint8_t *m = marr + 2u * pos;
            mn = (uint32_t)m[0] | ((uint32_t)m[1] << 8);
        }
    }
    d = d > 8u * PIX ? 8u * PIX : d;   // (a validated frame has none)
    // one scan for both sums: a row's depths total at most 64 * 16, its prefix bytes 511 * 16
    uint32_t sc = d | (pre << 16);
    for (uint32_t o = 1; o < mtx; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)sc, o, 64);
        if (lc >= o) sc += t;
    }
    const uint32_t last = lr * mtx + mtx - 1u;
    const uint32_t tot = (uint32_t)__shfl((int)sc, (int)(last < 63u ? last : 63u), 64);
    const uint32_t S = tot & 0xFFFFu, PRE = tot >> 16;   // the row's payload words, and those in front of it
    const uint32_t woff = (sc & 0xFFFFu) - d;            // payload words in front of this tile inside the row
    const uint32_t row_bytes = kPatchRowBytesOf(mtx, PIX);
    uint32_t *s_row = s_pay + lr * (row_bytes >> 2);     // (lanes of no row never use it)

    // ---- 2. the rows' payload ranges into LDS ----
    uint32_t sh = 0;
    if (row_has) {
        const uint8_t *src0 = pay + 8ull * ((uint64_t)base + PRE);
        const uint8_t *a_lo = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(src0) & ~(uintptr_t)15);
        sh = (uint32_t)(src0 - a_lo);
        const uint32_t nblk = (sh + 8u * S + 15u) >> 4;   // <= 4 * PIX * mtx + 1: row_bytes less the over-read
        const uint8_t *end = p.stream + p.stream_bytes;
        for (uint32_t i = lc; i < nblk; i += mtx) {
            const uint8_t *q = a_lo + 16u * i;
            uint4 v;
            if (q + 16 <= end) {
                const u32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(q));   // streamed once
                v = make_uint4(t.x, t.y, t.z, t.w);
            } else {   // the block that crosses the readable extent: only the bytes in front of it
                uint32_t wq[4] = {0, 0, 0, 0};
                for (uint32_t bb = 0; bb < 16u; bb++)
                    if (q + bb < end) wq[bb >> 2] |= (uint32_t)q[bb] << (8u * (bb & 3u));
                v = make_uint4(wq[0], wq[1], wq[2], wq[3]);
            }
            *reinterpret_cast<uint4 *>(s_row + 4u * i) = v;
        }
    }
    __syncthreads();

    // ---- 3. tile rows -> registers -> the band ----
    Row px[8];
    Row fillpx;
    if constexpr (PIX == 1u) {
        fillpx = make_uint2(p.fill * 0x01010101u, p.fill * 0x01010101u);
    } else {
        const uint32_t f2 = p.fill * 0x00010001u;
        fillpx = make_uint4(f2, f2, f2, f2);
    }
#pragma unroll
    for (uint32_t r = 0; r < 8u; r++) px[r] = fillpx;
    if (valid) {
        if constexpr (PIX == 1u) {
            const uint32_t mm = mn * 0x01010101u;
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                const uint32_t o = sh + 8u * woff + r * d;   // byte of tile row r (8d bits)
                const uint32_t w0 = o >> 2, s = o & 3u;
                const uint32_t a0 = s_row[w0], a1 = s_row[w0 + 1u], a2 = s_row[w0 + 2u];
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
                cut_row16(s_row + (a >> 2), s_row + (ah >> 2), a, ah, d, m32, mn2, px[r].x, px[r].y, px[r].z, px[r].w);
            }
        }
        // fill mode: the encoder's padding beyond W or H is not part of the frame
        const uint32_t ncol = (uint32_t)(p.W - 8 * tx), nrow = (uint32_t)((int64_t)p.H - 8 * ty);   // >= 1
        if (fill_mode && (ncol < 8u || nrow < 8u)) {
            // the dword holding pixels [a, a + 4 / PIX) of a tile row: which of its pixels lie left of column ncol
            auto keep = [&](uint32_t a) -> uint32_t {
                const uint32_t n = ncol > a ? ncol - a : 0u;
                return n >= 4u / PIX ? 0xFFFFFFFFu : (1u << (8u * PIX * n)) - 1u;
            };
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                if (r >= nrow) {
                    px[r] = fillpx;
                } else if constexpr (PIX == 1u) {
                    const uint32_t m0 = keep(0u), m1 = keep(4u);
                    px[r].x = (px[r].x & m0) | (fillpx.x & ~m0);
                    px[r].y = (px[r].y & m1) | (fillpx.y & ~m1);
                } else {
                    const uint32_t m0 = keep(0u), m1 = keep(2u), m2 = keep(4u), m3 = keep(6u);
                    px[r].x = (px[r].x & m0) | (fillpx.x & ~m0);
                    px[r].y = (px[r].y & m1) | (fillpx.x & ~m1);
                    px[r].z = (px[r].z & m2) | (fillpx.x & ~m2);
                    px[r].w = (px[r].w & m3) | (fillpx.x & ~m3);
                }
            }
        }
    }
    __syncthreads();   // every tile cut: the payload buffer becomes the band
    const uint32_t pitch = 8u * mtx;   // band row in pixels
    if (row_live && (valid || fill_mode)) {
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++)
            *reinterpret_cast<Row *>(reinterpret_cast<uint8_t *>(s_pay) + PIX * ((8u * lr + r) * pitch + 8u * lc)) = px[r];
    }
    __syncthreads();

    // ---- 4. the group's rows of the patch -> one output range (in pixels) ----
    constexpr uint32_t kPerDword = 4u / PIX, kPerBlock = 16u / PIX;
    const int64_t g_lo = 8 * tyg, g_hi = g_lo + 8 * (int64_t)p.G;
    const int64_t r_lo = g_lo > y ? g_lo : (int64_t)y, r_hi = g_hi < y_end ? g_hi : y_end;
    const uint32_t pw = (uint32_t)p.pw, nr = (uint32_t)(r_hi - r_lo);
    const uint32_t bx = (uint32_t)(x - 8 * tx_a), by = (uint32_t)(r_lo - g_lo);
    Pix *g = reinterpret_cast<Pix *>(p.out) + (pi * (size_t)p.ph + (size_t)(r_lo - y)) * (size_t)pw;
    const uint32_t len = nr * pw;
    const uintptr_t g0 = reinterpret_cast<uintptr_t>(g), a0 = g0 & ~(uintptr_t)15, g1 = g0 + PIX * len;
    const uint32_t nb = (uint32_t)((g1 - a0 + 15u) >> 4);
    for (uint32_t i = lane; i < nb; i += kPatchThreads) {
        const uintptr_t ba = a0 + 16u * i;
        const uint32_t lo = ba < g0 ? (uint32_t)(g0 - ba) / PIX : 0u;        // pixels of the block inside the range
        const uint32_t hi = ba + 16u > g1 ? (uint32_t)(g1 - ba) / PIX : kPerBlock;
        const uint32_t L = (uint32_t)(ba + PIX * lo - g0) / PIX;   // (row, column) of the first pixel, row-major at pitch pw
        uint32_t row = L / pw, col = L - row * pw;
        if (lo == 0u && hi == kPerBlock) {
            uint32_t v[4];
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                if (col + kPerDword <= pw) {
                    v[kk] = lds_u32_at(s_pay, PIX * ((by + row) * pitch + bx + col));
                    col += kPerDword;
                    if (col == pw) { col = 0; row++; }
                } else {   // a patch row ends inside the dword
                    uint32_t t = 0;
                    for (uint32_t bb = 0; bb < kPerDword; bb++) {
                        t |= (uint32_t)band[(by + row) * pitch + bx + col] << (8u * PIX * bb);
                        if (++col == pw) { col = 0; row++; }
                    }
                    v[kk] = t;
                }
            }
            u32x4_t o;
            o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
            __builtin_nontemporal_store(o, reinterpret_cast<u32x4_t *>(ba));   // the patch is written once
        } else {   // the range's first / last block: the pixels inside it only
            for (uint32_t bb = lo; bb < hi; bb++) {
                reinterpret_cast<Pix *>(ba)[bb] = band[(by + row) * pitch + bx + col];
                if (++col == pw) { col = 0; row++; }
            }
        }
    }
}

hipError_t launch_decode_patches(const PatchParams &p0, uint32_t n_frames, uint32_t pix, hipStream_t s) {
    const uint32_t total = n_frames * p0.n_patches * p0.groups;   // (the host keeps it below 2^31)
    PatchParams p = p0;
    // a grid of 2^26 workgroups or more is 2^32 work-items or more, which one launch does not take
    for (p.block0 = 0; p.block0 < total; p.block0 += kPatchMaxGrid) {
        const uint32_t grid = total - p.block0 < kPatchMaxGrid ? total - p.block0 : kPatchMaxGrid;
        if (pix == 1u)
            hipLaunchKernelGGL((decode_patches_kernel<1>), dim3(grid), dim3(kPatchThreads), 0, s, p);
        else
            hipLaunchKernelGGL((decode_patches_kernel<2>), dim3(grid), dim3(kPatchThreads), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dbde
