// dbde_proj_pipeline.h -- the front half of the projection kernels (gfx950, wave64; device code only).
//
// project_kernel, counts_kernel and lag_kernel share all of it: the piece of the window a workgroup takes (ProjPiece),
// the load pipeline that brings one (half) tile row per lane of a group of G frames into registers (ProjPipeline), and
// the cut of such a row into pixels (cut_row).  What a kernel does with the pixels is its own.
// gproject_kernel, wproject_kernel, pairs_kernel and rproject_kernel keep a prologue and a pipeline of their own (pairs
// and rproject walk two tile rows per frame) and take the small pieces from here: kProjWaves, readlane, pre_keep,
// pack_dms (pairs) and cut_row.  With these pieces their instruction streams are the ones they had; with proj_piece,
// ProjPipeline or load_row they are not, so load_row has ProjPipeline as its only caller so far.
//
// Everything is __forceinline__.  How a value is passed is part of what the kernels compile to (dbde_device.h,
// cut_row16): ProjPipeline refers to the kernel's own p, piece and buf as the kernels' lambdas captured them, and
// load_row / pack_dms take their scalars by value.  Each form was chosen by the listing: the other one changes the
// instruction count of the kernels.
#pragma once
#include "dbde_bits.h"
#include "dbde_device.h"
#include "dbde_project_kernels.h"

namespace dbde {

constexpr uint32_t kProjWaves = kProjThreads / 64u;

__device__ __forceinline__ uint32_t readlane(uint32_t v, uint32_t j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j); }

// The mask of the depth bytes [cb, cb + npre) of frame fb in lane tid's pre dword: those bytes are read as aligned
// dwords, lane tid < ndw holding dword tid.
__device__ __forceinline__ uint32_t pre_keep(const uint8_t *fb, const uint32_t &cb, const uint32_t &npre, const uint32_t &tid) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(fb + 24 + cb);
    const uint32_t head = (uint32_t)(a & 3u), ndw = (head + npre + 3u) >> 2;
    if (tid >= ndw) return 0u;
    const uint32_t lo = 4u * tid < head ? head - 4u * tid : 0u;   // bytes in front of cb
    const uint32_t hi = head + npre - 4u * tid;                   // bytes behind them, up to the piece's first tile
    return (hi >= 4u ? ~0u : (1u << (8u * hi)) - 1u) & ~((1u << (8u * lo)) - 1u);
}

// The three aligned dwords around the (half) row at src, a depth-d tile's, and sh = src's byte within the first.  A
// lane without need loads nothing and gets zeros.
template <uint32_t PIX>
__device__ __forceinline__ void load_row(const uint8_t *src, const uint8_t *end, bool need, uint32_t d,
                                         uint32_t hh, uint32_t &sh, uint32_t &a0, uint32_t &a1, uint32_t &a2) {
    sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
    const uint8_t *q8 = src - sh;   // (pointer arithmetic: the loads stay global ones)
    const bool tail = q8 + 12 > end;
    uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
    if (need && !tail) {
        const uint32_t *q32 = reinterpret_cast<const uint32_t *>(q8);
        w0 = q32[0]; w1 = q32[1]; w2 = q32[2];
    }
    if (need && tail) {   // the stream's last bytes: only those in front of stream_bytes (rare: its waits cost nothing)
        const uint32_t nb = PIX == 1u ? d : (4u * d + 4u * hh * (d & 1u) + 7u) >> 3;
        for (uint32_t b = sh; b < sh + nb; b++) {
            if (q8 + b >= end) break;
            const uint32_t v = (uint32_t)q8[b] << (8u * (b & 3u));
            if (b < 4u) w0 |= v; else if (b < 8u) w1 |= v; else w2 |= v;
        }
    }
    a0 = w0; a1 = w1; a2 = w2;
}

// What cut_row needs besides the dwords.  PIX 1: depth | minimum << 8 | byte shift << 16; PIX 2: depth | shift << 8 |
// minimum << 16 (ml / mh: its low / high byte).
template <uint32_t PIX>
__device__ __forceinline__ uint32_t pack_dms(uint32_t d, uint32_t sh, uint32_t ml, uint32_t mh) {
    if constexpr (PIX == 1u) return d | (ml << 8) | (sh << 16);
    else return d | (sh << 8) | (ml << 16) | (mh << 24);
}

// The row cut: load_row's dwords and pack_dms's word -> the lane's pixels with the minimum added, two dwords of four
// U8 (PIX 1: a tile row) or two U16 (PIX 2: half hh of a tile row) each.
template <uint32_t PIX>
__device__ __forceinline__ void cut_row(const uint32_t &a0, const uint32_t &a1, const uint32_t &a2, const uint32_t &dms,
                                        const uint32_t &hh, uint32_t &e0, uint32_t &e1) {
    if constexpr (PIX == 1u) {
        const uint32_t d = dms & 0xFFu, sh = dms >> 16;
        const uint32_t mm = ((dms >> 8) & 0xFFu) * 0x01010101u;
        const uint64_t bits = (uint64_t)__builtin_amdgcn_alignbyte(a1, a0, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(a2, a1, sh) << 32);
        uint32_t px[2];
        expand_row(bits, d, px[0], px[1]);
        e0 = add_bytes(px[0], mm);
        e1 = add_bytes(px[1], mm);
    } else {
        const uint32_t d = dms & 0xFFu, sh = (dms >> 8) & 0xFFu, so = 4u * hh * (d & 1u);
        const uint32_t m32 = d >= 16u ? 0xFFFFu : (1u << d) - 1u, mn2 = (dms >> 16) * 0x00010001u;
        const bool c2 = 2u * d >= 32u, c3 = 3u * d >= 32u;
        const uint32_t x0 = __builtin_amdgcn_alignbyte(a1, a0, sh);
        const uint32_t x1 = __builtin_amdgcn_alignbyte(a2, a1, sh);
        cut_four16(__builtin_amdgcn_alignbit(x1, x0, so), x1 >> so, d, m32, mn2, c2, c3, e0, e1);
    }
}

// One workgroup's piece and one lane's place in it.  The grid is (frame segment, window tile row, piece of
// kProjTilesOf(PIX) tiles); 8 * PIX lanes per tile, one per tile row (PIX 2: per half row).
template <uint32_t PIX>
struct ProjPiece {
    uint32_t tid, lane, wave;
    uint32_t t, r, hh;        // tile of the piece, row of the tile, half of the row (PIX 2)
    uint32_t seg;             // the frame segment
    uint32_t ty, txp;         // the tile row, the piece's first tile column
    bool has_tile;            // t is a tile of the window
    uint32_t pos0, c, cb;     // the piece's first tile (stream order), its chunk, that chunk's first tile
    uint32_t npre, cstride;   // pos0 - cb, < 512 (roi_index_geometry); chunk_off words per frame
};

template <uint32_t PIX, class Params>
__device__ __forceinline__ ProjPiece<PIX> proj_piece(const Params &p) {
    constexpr uint32_t kTiles = kProjTilesOf(PIX);
    ProjPiece<PIX> pc;
    const uint32_t tid = threadIdx.x;
    pc.tid = tid; pc.lane = tid & 63u; pc.wave = tid >> 6;
    pc.t = PIX == 1u ? tid >> 3 : tid >> 4; pc.r = PIX == 1u ? tid & 7u : (tid >> 1) & 7u; pc.hh = PIX == 1u ? 0u : tid & 1u;
    const uint32_t per_seg = p.rows * p.pieces;
    pc.seg = blockIdx.x / per_seg;
    const uint32_t rem = blockIdx.x - pc.seg * per_seg;
    const uint32_t br = rem / p.pieces, col = rem - br * p.pieces;
    pc.ty = p.ty0 + br; pc.txp = p.tx0 + col * kTiles;
    const uint32_t tx_b = (uint32_t)(p.x0 + p.rw - 1) >> 3;
    const uint32_t nt = tx_b + 1u - pc.txp < kTiles ? tx_b + 1u - pc.txp : kTiles;
    pc.has_tile = pc.t < nt;
    pc.pos0 = pc.ty * p.w + pc.txp;
    pc.c = dec_chunk_of(p.geom, pc.pos0); pc.cb = dec_chunk_begin(p.geom, pc.c);
    pc.npre = pc.pos0 - pc.cb;
    pc.cstride = p.geom.cpf + 1u;
    return pc;
}

// The load pipeline of a piece.  Three stages are in flight per group of G frames, each a call ahead of the next:
// the per-frame words (Words: lane k < G holds the group's frame k), the depth / minimum loads (Meta) and the payload
// loads (Pay; one barrier per group, for the offsets scan).  A kernel declares s_wsum and the stage variables, and
// calls the stages in the order its walk needs.
struct ProjWords {
    uint32_t ok, base;
    uint64_t fo;
};
template <uint32_t G>
struct ProjMeta {
    uint32_t ok[G];            // uniform: frame accepted (and inside the segment)
    uint32_t base[G];          // uniform: payload words of the frame in front of the piece's chunk
    const uint8_t *fb[G];      // uniform: the frame
    uint32_t d8[G], ml[G], mh[G];   // depth, minimum (PIX 2: its low / high byte) of this lane's tile (raw loads)
    uint32_t pre[G];           // this lane's dword of the depth bytes in front of the piece (masked where used)
};
template <uint32_t G>
struct ProjPay {
    uint32_t a0[G], a1[G], a2[G];   // the aligned dwords around this lane's (half) row
    uint32_t dms[G];                // pack_dms
};

template <uint32_t PIX, uint32_t G, class Params>
struct ProjPipeline {
    typedef ProjWords Words;
    typedef ProjMeta<G> Meta;
    typedef ProjPay<G> Pay;
    static constexpr uint32_t kDmax = 8u * PIX;

    const Params &p;
    const ProjPiece<PIX> &pc;
    uint32_t (&s_wsum)[2][G][2][kProjWaves];   // per group of frames (double-buffered): wave depth totals, sums in front
    const uint8_t *const end;                  // p.stream + p.stream_bytes
    uint32_t &buf;                             // which half of s_wsum the next group takes

    // the words of frames g0 + k < f_end
    __device__ __forceinline__ void issue_words(Words &wd, uint32_t g0, const uint32_t &f_end) const {
        const uint32_t g = g0 + (pc.lane < G ? pc.lane : 0u);
        wd.ok = 0u; wd.base = 0u; wd.fo = 0u;
        if (pc.lane < G && g < f_end) {
            wd.ok = p.frame_ok[g];
            wd.fo = p.frame_offsets[g];
            wd.base = p.chunk_off[(size_t)g * pc.cstride + pc.c];
        }
    }

    // pre: depth bytes [cb, pos0) of the frame, as aligned dwords, lane tid < ndw holding dword tid.  Every load is
    // unconditional inside an accepted frame (lanes without a tile read tile 0, lanes past ndw dword 0) and nothing
    // consumes a loaded value here, so that the loads stay in flight while the kernel works on the group in front.
    // The U16 minima start at 28 + T, possibly at an odd address: read byte by byte.
    __device__ __forceinline__ void issue_meta(Meta &m, const Words &wd) const {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            m.ok[k] = 0u; m.base[k] = 0u; m.fb[k] = p.stream; m.d8[k] = 0u; m.ml[k] = 0u; m.mh[k] = 0u; m.pre[k] = 0u;
            m.ok[k] = readlane(wd.ok, k);   // 0 past the segment
            if (m.ok[k]) {
                const uint64_t fo = (uint64_t)readlane((uint32_t)wd.fo, k) | ((uint64_t)readlane((uint32_t)(wd.fo >> 32), k) << 32);
                m.fb[k] = p.stream + fo;   // validated: the whole frame lies inside stream_bytes
                m.base[k] = readlane(wd.base, k);
                const uint8_t *darr = m.fb[k] + 24;
                const uint32_t tt = pc.has_tile ? pc.t : 0u;
                m.d8[k] = darr[pc.pos0 + tt];
                if constexpr (PIX == 1u) {
                    m.ml[k] = darr[4u + p.T + pc.pos0 + tt];
                } else {
                    m.ml[k] = darr[4u + p.T + 2u * (pc.pos0 + tt)];
                    m.mh[k] = darr[5u + p.T + 2u * (pc.pos0 + tt)];
                }
                const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(darr + pc.cb) & 3u), ndw = (head + pc.npre + 3u) >> 2;
                const uint8_t *a_lo = darr + pc.cb - head;   // (pointer arithmetic: the load stays a global one)
                m.pre[k] = *reinterpret_cast<const uint32_t *>(a_lo + 4u * (pc.tid < ndw ? pc.tid : 0u));   // inside the frame
            }
        }
    }

    // the group's tile offsets (one barrier) and its payload loads
    __device__ __forceinline__ void issue_payload(const Meta &m, Pay &q) {
        uint32_t any = 0;
#pragma unroll
        for (uint32_t k = 0; k < G; k++) any |= m.ok[k];
        if (!any) {
#pragma unroll
            for (uint32_t k = 0; k < G; k++) { q.a0[k] = q.a1[k] = q.a2[k] = 0u; q.dms[k] = 0u; }
            return;
        }
        uint32_t incl[G];
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            const uint32_t d = pc.has_tile ? (m.d8[k] > kDmax ? kDmax : m.d8[k]) : 0u;   // (a validated frame has none above)
            incl[k] = wave_scan_incl((PIX == 1u ? pc.r == 0u : (pc.tid & 15u) == 0u) ? d : 0u);   // the tile's first lane
            const uint32_t pw = wave_sum(__builtin_amdgcn_sad_u8(m.pre[k] & pre_keep(m.fb[k], pc.cb, pc.npre, pc.tid), 0u, 0u));
            if (pc.lane == 63u) s_wsum[buf][k][0][pc.wave] = incl[k];
            if (pc.lane == 0u) s_wsum[buf][k][1][pc.wave] = pw;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            uint32_t wbase = 0, PRE = 0;
#pragma unroll
            for (uint32_t w = 0; w < kProjWaves; w++) {
                wbase += w < pc.wave ? s_wsum[buf][k][0][w] : 0u;
                PRE += s_wsum[buf][k][1][w];
            }
            const uint32_t d = pc.has_tile ? (m.d8[k] > kDmax ? kDmax : m.d8[k]) : 0u;
            const uint32_t woff = m.base[k] + PRE + wbase + incl[k] - d;   // payload words in front of the tile
            // PIX 2, the half row: byte r * d + h * (d / 2), a nibble further when d is odd; 4d bits (+ 4) <= 8 bytes
            const uint8_t *src = m.fb[k] + 32 + (PIX + 1ull) * p.T + 8ull * woff + pc.r * d + pc.hh * (d >> 1);
            const bool need = m.ok[k] && pc.has_tile && d != 0u;
            uint32_t sh;
            load_row<PIX>(src, end, need, d, pc.hh, sh, q.a0[k], q.a1[k], q.a2[k]);
            q.dms[k] = pack_dms<PIX>(d, sh, m.ml[k], m.mh[k]);
        }
        buf ^= 1u;
    }
};

}  // namespace dbde
