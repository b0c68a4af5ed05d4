// dbde_rproject_kernels.hip -- registered projections for MI355X (gfx950, wave64): project's per-pixel maximum, minimum,
// sum and sum of squares over a batch of frames, of an rw x rh window whose origin is given per frame (one integer
// (x, y) per frame, clamped into the frame as the window decoder clamps), straight from the compressed bytes (no image
// is written).  DESIGN.md 4.22.
//
// rproject_kernel<STATS, PIX>: STATS = 3, 12 or 15 (kRProjInstanceOf: a superset of the requested statistics; a plane
// that is not requested is accumulated and not stored), PIX = 1 for DBDE frames, PIX = 2 for DBDE16 frames.  One
// 256-lane workgroup per (frame segment, band of 8 OUTPUT rows, piece of kRProjColsOf(PIX) OUTPUT columns).  The
// lanes are project_kernel's: lane (t, r) is tile t of the piece and row r of the band (PIX 2: and half h of the row),
// and it decodes exactly one 8-pixel (half: 4-pixel) row per frame, so the payload traffic is 1x.
//
// The front: per-frame geometry.  For frame f with clamped origin (x, y) the piece's source columns start at
// X = x + piece offset, in tile X >> 3 at residue sx = X & 7, and the band's source rows at Y = y + 8 * band, in tile
// row ty = Y >> 3 at residue sy = Y & 7.  Output row r is row (sy + r) & 7 of tile row ty + ((sy + r) >> 3): with
// sy != 0 the band spans two tile rows, and the workgroup runs project's prefix (the chunk's payload offset, the depth
// bytes in front within the chunk, the scan over the piece's tiles) for both through the same barrier; each lane then
// takes the offset of the tile row its output row lies in.  Lane k < 4 of every wave computes the words of frame k of
// a group (ok, offset, the two chunk offsets, first tile, depth bytes in front, residues); they are broadcast with
// v_readlane where they are used, as uniforms.  Output rows past rh take the band's last row inside the window, tiles
// past the piece's last source tile take its first: every load lies inside an accepted frame, and a tile row below the
// band's last source row is never read.
//
// The columns.  Every lane writes its decoded row into a band in LDS, [frame of the group][row][68 dwords], and after
// the group's one barrier reads its 8 (4) output pixels back at byte 8 * slot + PIX * sx through three dwords and two
// byte-aligns.  A piece of kProjTilesOf(PIX) source tiles therefore owns 8 * (kProjTilesOf(PIX) - 1) output columns;
// the lanes of the last slots own nothing.
//
// The accumulators, the per-segment partials and the combine kernel are project's.
#include "dbde_rproject_kernels.h"

#include <type_traits>

#include "dbde_proj_pipeline.h"

namespace dbde {

namespace {

template <uint32_t PIX> using RProjPix = typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type;
template <uint32_t PIX> using RProjSq = typename std::conditional<PIX == 1u, uint32_t, uint64_t>::type;

// Frames of [0, p.n_frames) that the index accepted -> *p.out_count (added to it when accumulating).  Whole workgroup.
__device__ void write_count(const ProjParams &p) {
    __shared__ uint32_t s_c[kProjWaves];
    const uint32_t tid = threadIdx.x;
    uint32_t c = 0;
    for (uint32_t g = tid; g < p.n_frames; g += kProjThreads) c += p.frame_ok[g] != 0u ? 1u : 0u;
    c = wave_sum(c);
    if ((tid & 63u) == 0u) s_c[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        uint64_t total = 0;
        for (uint32_t k = 0; k < kProjWaves; k++) total += s_c[k];
        *p.out_count = (p.accumulate ? *p.out_count : 0ull) + total;
    }
}

// The per-frame words of the front, one frame per lane.  geo: sx | sy << 3 | below << 6 | source tiles << 8.
struct RFrameWords {
    uint32_t ok;
    uint64_t fo;
    uint32_t base[2];    // payload words of the frame in front of the chunk of the band's first / second tile row
    uint32_t pos0;       // the piece's first source tile (stream order) in the band's first tile row
    uint32_t npre[2];    // tiles between that chunk's first tile and the piece's first tile (< 512), per tile row
    uint32_t geo;
};

// The piece (output columns [ocol0, ocol0 + ncols)) and band (output rows from 8 * br, the last one inside the window
// rlast rows further) of one workgroup.
struct RPiece {
    uint32_t ocol0, ncols, orow0, rlast;
};

// The front, separable from the reduction behind it: frame g's words for one piece.  The origin of a rejected frame is
// not read.  Any int32 origin is legal: the clamp is the window decoder's.
__device__ __forceinline__ void rproject_frame_words(const RProjParams &rp, const RPiece &pc, uint32_t g, bool first_piece,
                                                     RFrameWords &wd) {
    const ProjParams &p = rp.pj;
    wd.ok = p.frame_ok[g];
    wd.fo = p.frame_offsets[g];
    wd.base[0] = wd.base[1] = 0u; wd.pos0 = 0u; wd.npre[0] = wd.npre[1] = 0u; wd.geo = 0u;
    if (!wd.ok) return;
    int x = rp.origins[2u * (size_t)g], y = rp.origins[2u * (size_t)g + 1u];
    x = x < 0 ? 0 : (x > rp.W - p.rw ? rp.W - p.rw : x);
    y = y < 0 ? 0 : (y > rp.H - p.rh ? rp.H - p.rh : y);
    if (first_piece && rp.origins_used) {
        rp.origins_used[2u * (size_t)g] = x;
        rp.origins_used[2u * (size_t)g + 1u] = y;
    }
    const uint32_t X = (uint32_t)x + pc.ocol0, Y = (uint32_t)y + pc.orow0;
    const uint32_t txp = X >> 3, sx = X & 7u, ty = Y >> 3, sy = Y & 7u;
    const uint32_t nt = ((X + pc.ncols - 1u) >> 3) - txp + 1u;          // <= kProjTilesOf(pix), inside the frame
    const uint32_t below = ((Y + pc.rlast) >> 3) != ty ? 1u : 0u;       // the band reaches into tile row ty + 1 (< h)
    const uint32_t cstride = p.geom.cpf + 1u;
    wd.pos0 = ty * p.w + txp;
    wd.geo = sx | (sy << 3) | (below << 6) | (nt << 8);
#pragma unroll
    for (uint32_t rr = 0; rr < 2u; rr++) {
        if (rr && !below) continue;
        const uint32_t pos = wd.pos0 + rr * p.w;
        const uint32_t ch = dec_chunk_of(p.geom, pos);
        wd.npre[rr] = pos - dec_chunk_begin(p.geom, ch);
        wd.base[rr] = p.chunk_off[(size_t)g * cstride + ch];
    }
}

}  // namespace

template <uint32_t STATS, uint32_t PIX>
__global__ __launch_bounds__(kProjThreads) void rproject_kernel(RProjParams rp) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    typedef RProjPix<PIX> Pix;
    const ProjParams &p = rp.pj;
    constexpr bool kMax = (STATS & kProjMax) != 0u, kMin = (STATS & kProjMin) != 0u;
    constexpr bool kSum = (STATS & kProjSum) != 0u, kSq = (STATS & kProjSumSq) != 0u;
    constexpr uint32_t G = kRProjGroup, kDmax = 8u * PIX, kNpx = 8u / PIX;   // kNpx: pixels per lane
    constexpr uint32_t kCols = kRProjColsOf(PIX), kOwnedSlots = kCols / kNpx, kRowDw = kRProjRowDwords;
    constexpr uint32_t kPixMask = PIX == 1u ? 0xFFu : 0xFFFFu;
    __shared__ uint32_t s_wsum[2][G][2][2][kProjWaves];   // per group of frames (double-buffered), per tile row: wave depth totals, sums in front
    __shared__ __attribute__((aligned(8))) uint32_t s_band[2][G][kRProjBandRows][kRowDw];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // tile of the piece, row of the band, half of the row (PIX 2)
    const uint32_t t = PIX == 1u ? tid >> 3 : tid >> 4, r = PIX == 1u ? tid & 7u : (tid >> 1) & 7u, hh = PIX == 1u ? 0u : tid & 1u;
    const uint32_t slot = PIX == 1u ? t : 2u * t + hh;   // the lane's two dwords of a band row: 2 * slot
    const uint32_t per_seg = p.rows * p.pieces;
    const uint32_t seg = blockIdx.x / per_seg;
    const uint32_t rem = blockIdx.x - seg * per_seg;
    const uint32_t br = rem / p.pieces, pcx = rem - br * p.pieces;
    RPiece piece;
    piece.ocol0 = pcx * kCols;
    piece.ncols = (uint32_t)p.rw - piece.ocol0 < kCols ? (uint32_t)p.rw - piece.ocol0 : kCols;   // >= 1
    piece.orow0 = br * kRProjBandRows;
    piece.rlast = (uint32_t)p.rh - 1u - piece.orow0 < 7u ? (uint32_t)p.rh - 1u - piece.orow0 : 7u;
    const uint32_t rc = r < piece.rlast ? r : piece.rlast;   // the band row this lane decodes (its own inside the window)
    const uint32_t f_begin = seg * p.fps;
    const uint64_t f_last = (uint64_t)f_begin + p.fps;
    const uint32_t f_end = f_last < p.n_frames ? (uint32_t)f_last : p.n_frames;
    const uint8_t *const end = p.stream + p.stream_bytes;

    // ---- accumulators: this lane's kNpx output pixels (project_kernel's) ----
    uint32_t mx[2] = {0u, 0u}, mxo[2] = {0u, 0u};
    uint32_t mn[2] = {~0u, ~0u}, mno[2] = {~0u, ~0u};
    uint32_t sum[kNpx] = {};
    RProjSq<PIX> sq[kNpx] = {};

    // ---- the per-frame words of a group, one group ahead of their use: lane k < G holds frame g0 + k ----
    auto issue_words = [&](RFrameWords &wd, uint32_t g0) __attribute__((always_inline)) {
        const uint32_t g = g0 + (lane < G ? lane : 0u);
        wd.ok = 0u; wd.fo = 0u; wd.base[0] = wd.base[1] = 0u; wd.pos0 = 0u; wd.npre[0] = wd.npre[1] = 0u; wd.geo = 0u;
        if (lane < G && g < f_end) rproject_frame_words(rp, piece, g, rem == 0u && wave == 0u, wd);
    };

    // ---- one group of frames in flight ----
    struct Meta {
        RFrameWords w;             // lane k: frame k of the group (read as uniforms with readlane)
        uint32_t d8[2][G];         // depth of this lane's tile in the band's first / second tile row (raw loads)
        uint32_t ml[G], mh[G];     // minimum (PIX 2: its low / high byte) of this lane's tile in ITS tile row
        uint32_t pre[2][G];        // this lane's dword of the depth bytes in front of the piece, per tile row (masked where used)
    };
    struct Pay {
        uint32_t a0[G], a1[G], a2[G];   // the aligned dwords around this lane's (half) row
        uint32_t dms[G];                // PIX 1: depth | minimum << 8 | byte shift << 16; PIX 2: depth | shift << 8 | minimum << 16
    };
    auto frame_of = [&](const RFrameWords &w, uint32_t k) __attribute__((always_inline)) -> const uint8_t * {
        const uint64_t fo = (uint64_t)readlane((uint32_t)w.fo, k) | ((uint64_t)readlane((uint32_t)(w.fo >> 32), k) << 32);
        return p.stream + fo;   // validated: the whole frame lies inside stream_bytes
    };

    // Every load is unconditional inside an accepted frame (lanes without a tile read the piece's first tile, lanes
    // past ndw dword 0) and nothing consumes a loaded value here, so that the loads stay in flight while the group in
    // front is accumulated.  The U16 minima start at 28 + T, possibly at an odd address: read byte by byte.
    auto issue_meta = [&](Meta &m, const RFrameWords &wd) __attribute__((always_inline)) {
        m.w = wd;
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            m.d8[0][k] = m.d8[1][k] = 0u; m.ml[k] = 0u; m.mh[k] = 0u; m.pre[0][k] = m.pre[1][k] = 0u;
            if (readlane(wd.ok, k)) {   // 0 past the segment
                const uint8_t *darr = frame_of(wd, k) + 24;
                const uint32_t geo = readlane(wd.geo, k), pos0 = readlane(wd.pos0, k);
                const uint32_t sy = (geo >> 3) & 7u, below = (geo >> 6) & 1u, nt = geo >> 8;
                const uint32_t tt = t < nt ? t : 0u;
                const uint32_t posm = pos0 + tt + ((sy + rc) >> 3) * p.w;   // this lane's tile
                if constexpr (PIX == 1u) {
                    m.ml[k] = darr[4u + p.T + posm];
                } else {
                    m.ml[k] = darr[4u + p.T + 2u * posm];
                    m.mh[k] = darr[5u + p.T + 2u * posm];
                }
#pragma unroll
                for (uint32_t rr = 0; rr < 2u; rr++) {
                    if (rr && !below) continue;
                    const uint32_t pos = pos0 + rr * p.w, npre = readlane(wd.npre[rr], k), cb = pos - npre;
                    m.d8[rr][k] = darr[pos + tt];
                    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(darr + cb) & 3u), ndw = (head + npre + 3u) >> 2;
                    const uint8_t *a_lo = darr + cb - head;   // (pointer arithmetic: the load stays a global one)
                    m.pre[rr][k] = *reinterpret_cast<const uint32_t *>(a_lo + 4u * (tid < ndw ? tid : 0u));   // inside the frame
                }
            }
        }
    };
    // the group's tile offsets (the group's one barrier, which also publishes the band written in front of it) and its
    // payload loads
    uint32_t buf = 0;
    auto issue_payload = [&](const Meta &m, Pay &q) __attribute__((always_inline)) {
        uint32_t any = 0;
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            any |= readlane(m.w.ok, k);
            q.a0[k] = q.a1[k] = q.a2[k] = 0u; q.dms[k] = 0u;
        }
        if (!any) {
            __syncthreads();
            return;
        }
        uint32_t incl0[G], incl1[G];   // the scans of the band's first / second tile row
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            incl0[k] = incl1[k] = 0u;
            if (!readlane(m.w.ok, k)) continue;
            const uint8_t *fb = frame_of(m.w, k);
            const uint32_t geo = readlane(m.w.geo, k), pos0 = readlane(m.w.pos0, k);
            const uint32_t below = (geo >> 6) & 1u, nt = geo >> 8;
#pragma unroll
            for (uint32_t rr = 0; rr < 2u; rr++) {
                if (rr && !below) continue;
                const uint32_t npre = readlane(m.w.npre[rr], k), cb = pos0 + rr * p.w - npre;
                const uint32_t d = t < nt ? (m.d8[rr][k] > kDmax ? kDmax : m.d8[rr][k]) : 0u;   // (a validated frame has none above)
                const uint32_t sc = wave_scan_incl((PIX == 1u ? r == 0u : (tid & 15u) == 0u) ? d : 0u);   // the tile's first lane
                if (rr) incl1[k] = sc; else incl0[k] = sc;
                const uint32_t pw = wave_sum(__builtin_amdgcn_sad_u8(m.pre[rr][k] & pre_keep(fb, cb, npre, tid), 0u, 0u));
                if (lane == 63u) s_wsum[buf][k][rr][0][wave] = sc;
                if (lane == 0u) s_wsum[buf][k][rr][1][wave] = pw;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!readlane(m.w.ok, k)) continue;
            const uint8_t *fb = frame_of(m.w, k);
            const uint32_t geo = readlane(m.w.geo, k);
            const uint32_t sy = (geo >> 3) & 7u, nt = geo >> 8;
            const uint32_t rr = (sy + rc) >> 3, trow = (sy + rc) & 7u;   // this lane's tile row of the band, its row of the tile
            uint32_t wbase = 0, PRE = 0;
#pragma unroll
            for (uint32_t w = 0; w < kProjWaves; w++) {
                wbase += w < wave ? s_wsum[buf][k][rr][0][w] : 0u;
                PRE += s_wsum[buf][k][rr][1][w];
            }
            const uint32_t sel = 0u - rr;   // all ones in the second tile row
            const uint32_t draw = (m.d8[0][k] & ~sel) | (m.d8[1][k] & sel), incl = (incl0[k] & ~sel) | (incl1[k] & sel);
            const uint32_t d = t < nt ? (draw > kDmax ? kDmax : draw) : 0u;
            const uint32_t base = (readlane(m.w.base[0], k) & ~sel) | (readlane(m.w.base[1], k) & sel);
            const uint32_t woff = base + PRE + wbase + incl - d;   // payload words in front of the tile
            // PIX 2, the half row: byte trow * d + h * (d / 2), a nibble further when d is odd; 4d bits (+ 4) <= 8 bytes
            const uint8_t *src = fb + 32 + (PIX + 1ull) * p.T + 8ull * woff + trow * d + hh * (d >> 1);
            const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
            const uint8_t *q8 = src - sh;   // (pointer arithmetic: the loads stay global ones)
            const bool need = t < nt && d != 0u, tail = q8 + 12 > end;
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
            q.a0[k] = w0; q.a1[k] = w1; q.a2[k] = w2;
            if constexpr (PIX == 1u) q.dms[k] = d | (m.ml[k] << 8) | (sh << 16);
            else q.dms[k] = d | (sh << 8) | (m.ml[k] << 16) | (m.mh[k] << 24);
        }
        buf ^= 1u;
    };

    // the group's decoded rows -> the band (in front of the group's barrier)
    uint32_t bb = 0;
    auto stage = [&](const Meta &m, const Pay &q) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!readlane(m.w.ok, k)) continue;   // rejected (or past the segment): contributes nothing
            uint32_t v0, v1;
            cut_row<PIX>(q.a0[k], q.a1[k], q.a2[k], q.dms[k], hh, v0, v1);
            *reinterpret_cast<uint2 *>(&s_band[bb][k][r][2u * slot]) = make_uint2(v0, v1);
        }
    };
    // the band (behind the group's barrier), re-aligned to the output columns -> the accumulators
    auto consume = [&](const Meta &m) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!readlane(m.w.ok, k)) continue;
            const uint32_t sb = PIX * (readlane(m.w.geo, k) & 7u);   // bytes the output columns lie behind the tiles'
            const uint32_t *const row = &s_band[bb][k][r][2u * slot + (sb >> 2)];
            const uint32_t w0 = row[0], w1 = row[1], w2 = row[2];
            uint32_t px[2];
            px[0] = __builtin_amdgcn_alignbyte(w1, w0, sb & 3u);
            px[1] = __builtin_amdgcn_alignbyte(w2, w1, sb & 3u);
            if constexpr (PIX == 1u) {
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint32_t e = px[h] & 0x00FF00FFu;
                    if (kMax) { mx[h] = pk_max_u16(mx[h], e); mxo[h] = pk_max_u16(mxo[h], px[h]); }
                    if (kMin) { mn[h] = pk_min_u16(mn[h], e); mno[h] = pk_min_u16(mno[h], px[h]); }
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t v = (px[h] >> (8 * i)) & 0xFFu;
                        if (kSum) sum[4 * h + i] += v;
                        if (kSq) sq[4 * h + i] += v * v;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    if (kMax) mx[j] = pk_max_u16(mx[j], px[j]);
                    if (kMin) mn[j] = pk_min_u16(mn[j], px[j]);
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const uint32_t v = (px[j] >> (16 * i)) & 0xFFFFu;
                        if (kSum) sum[2 * j + i] += v;
                        if (kSq) sq[2 * j + i] += (uint64_t)(v * v);   // v * v < 2^32; the add carries into the high dword
                    }
                }
            }
        }
        bb ^= 1u;
    };

    // ---- the pipeline: accumulate group k while group k + 1's payload and group k + 2's depth bytes load ----
    Meta m_cur, m_nxt, m_nn;
    Pay q_cur, q_nxt;
    RFrameWords w_nn;
    issue_words(w_nn, f_begin);
    issue_meta(m_cur, w_nn);
    issue_payload(m_cur, q_cur);
    issue_words(w_nn, f_begin + G);
    issue_meta(m_nxt, w_nn);
    issue_words(w_nn, f_begin + 2u * G);
    for (uint32_t g0 = f_begin; g0 < f_end; g0 += G) {
        stage(m_cur, q_cur);
        issue_payload(m_nxt, q_nxt);   // (the barrier between stage and consume)
        issue_meta(m_nn, w_nn);
        issue_words(w_nn, g0 + 3u * G);
        consume(m_cur);
        m_cur = m_nxt;
        q_cur = q_nxt;
        m_nxt = m_nn;
    }

    // ---- the owned output pixels of this lane -> the requested planes, or this segment's partials ----
    Pix *const out_max = reinterpret_cast<Pix *>(p.out_max), *const out_min = reinterpret_cast<Pix *>(p.out_min);
    const uint32_t orow = piece.orow0 + r;
    if (slot < kOwnedSlots && orow < (uint32_t)p.rh) {
        const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
        const uint64_t row0 = (uint64_t)orow * (uint64_t)p.rw;
        const bool direct = p.segments == 1u;
#pragma unroll
        for (int i = 0; i < (int)kNpx; i++) {
            const uint32_t oc = piece.ocol0 + kNpx * slot + (uint32_t)i;
            if (oc >= (uint32_t)p.rw) continue;
            const uint64_t o = row0 + oc, ow = (uint64_t)seg * P + o;
            // pixel i of a packed max / min: PIX 1 byte i & 3 of the even / odd accumulator, PIX 2 U16 i & 1 of a pair
            const int h = PIX == 1u ? i >> 2 : i >> 1, sb = PIX == 1u ? 8 * (i & 3) : 16 * (i & 1);
            if (kMax && out_max) {
                uint32_t v = ((PIX == 1u && (i & 1)) ? mxo[h] : mx[h]) >> sb & kPixMask;
                if (direct) {
                    if (p.accumulate) { const uint32_t ov = out_max[o]; v = v > ov ? v : ov; }
                    out_max[o] = (Pix)v;
                } else {
                    reinterpret_cast<Pix *>(p.ws_max)[ow] = (Pix)v;
                }
            }
            if (kMin && out_min) {
                uint32_t v = ((PIX == 1u && (i & 1)) ? mno[h] : mn[h]) >> sb & kPixMask;
                if (direct) {
                    if (p.accumulate) { const uint32_t ov = out_min[o]; v = v < ov ? v : ov; }
                    out_min[o] = (Pix)v;
                } else {
                    reinterpret_cast<Pix *>(p.ws_min)[ow] = (Pix)v;
                }
            }
            if (kSum && p.out_sum) {
                if (direct) p.out_sum[o] = (p.accumulate ? p.out_sum[o] : 0ull) + sum[i];
                else p.ws_sum[ow] = sum[i];
            }
            if (kSq && p.out_sumsq) {
                if (direct) p.out_sumsq[o] = (p.accumulate ? p.out_sumsq[o] : 0ull) + sq[i];
                else reinterpret_cast<RProjSq<PIX> *>(p.ws_sumsq)[ow] = sq[i];
            }
        }
    }
    if (p.segments == 1u && blockIdx.x == 0u) write_count(p);
}

typedef void (*RProjKernel)(RProjParams);

hipError_t launch_rproject(const RProjParams &p, uint32_t stats, uint32_t pix, hipStream_t s) {
    if (stats < 1u || stats > kProjAll || (pix != 1u && pix != 2u) || !p.origins) return hipErrorInvalidValue;
    const uint32_t inst = kRProjInstanceOf(stats);
    RProjKernel k;
    if (pix == 1u) k = inst == 3u ? rproject_kernel<3, 1> : inst == 12u ? rproject_kernel<12, 1> : rproject_kernel<15, 1>;
    else k = inst == 3u ? rproject_kernel<3, 2> : inst == 12u ? rproject_kernel<12, 2> : rproject_kernel<15, 2>;
    const uint32_t grid = p.pj.pieces * p.pj.rows * p.pj.segments;   // (the host keeps it below 2^31)
    hipLaunchKernelGGL(k, dim3(grid), dim3(kProjThreads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.pj.segments == 1u) return e;
    return launch_project_combine(p.pj, pix, s);
}

}  // namespace dbde
