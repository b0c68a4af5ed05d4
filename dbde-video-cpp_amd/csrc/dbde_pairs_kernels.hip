// dbde_pairs_kernels.hip -- neighbour-product projections for MI355X (gfx950, wave64): one U64 plane per requested
// forward offset (dx, dy) of the rw x rh window, out[j][y][x] = sum over the accepted frames of
// p[y][x] * p[y + dy][x + dx] where both pixels lie inside the window, straight from the compressed bytes (no image is
// written).  DESIGN.md 4.20.
//
// pairs_kernel<MASK, PIX>: MASK = 1, 3 or 15, the instance's offsets (kPairsInstanceOf), PIX = 1 for DBDE frames,
// PIX = 2 for DBDE16 frames.  The launch shape and the load pipeline are project_kernel's (dbde_proj_pipeline.h),
// as counts_kernel took them: one 256-lane workgroup per (frame segment, window tile row, piece), one lane per tile
// row (PIX 2: per half row), the segment's frames walked in groups of kPairsGroup with the payload loads of group
// k + 1, the depth / minimum loads of group k + 2 and the per-frame words of group k + 3 in flight while group k is
// multiplied, one barrier per group.  The body is this file's own.
//
// The halo.  A lane's partner pixels lie in other lanes, other waves, the next piece and the next tile row:
//   * Inside the workgroup every lane writes its decoded (half) row of each frame of the group into a band in LDS,
//     [frame][row 0..8][72 dwords], and after the group's one barrier reads its own row, the dword to its right and the
//     four dwords around it in the row below.  Lane and wave boundaries disappear in the addressing.
//   * Across pieces: pieces overlap.  A workgroup decodes kProjTilesOf(PIX) tiles and owns the pairs whose FIRST pixel
//     lies in all but the first (DOWN_LEFT) and the last (RIGHT, DOWN_RIGHT) of them; the window's first and last piece
//     own their outer tile too, whose partners beyond lie outside the window.  Every pair has one owner.
//   * Across tile rows: row 7 pairs with row 0 of tile row ty + 1, whose tiles start w tiles further on in the stream,
//     in general in another index chunk.  The workgroup runs a second prefix for that row (its chunk's offset, the
//     depth bytes in front, the scan over its tiles) through the same pipeline and barrier, and the lanes of tile row 0
//     load and decode that one row into band row 8.  The window's last tile row has no row below and skips it.
// The guard dwords and the slots of lanes without a tile hold whatever they hold: they are partners only of elements
// whose partner lies outside the window, which are never stored.
//
// The value.  The sums are integers: U32 per lane for DBDE (65,536 frames * 255^2 < 2^32, kProjMaxFramesPerSegment),
// U64 for DBDE16.  With one segment each owned lane writes its window pixels of the requested planes (old + sum when
// accumulating; an element without a partner gets 0, or stays when accumulating); with more, the per-segment partials
// [segments][planes][rw * rh] go to the workspace and pairs_combine_kernel adds them onto the prior content
// (accumulate) or onto 0.
#include "dbde_pairs_kernels.h"

#include <type_traits>

#include "dbde_proj_pipeline.h"

namespace dbde {

namespace {

// Frames of [0, p.n_frames) that the index accepted -> *p.out_count (added to it when accumulating).  Whole workgroup.
__device__ void write_count(const PairsParams &p) {
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

constexpr uint32_t popc(uint32_t v) { return (v & 1u) + ((v >> 1) & 1u) + ((v >> 2) & 1u) + ((v >> 3) & 1u); }
// (dx, dy) of offset bit b
constexpr int kDx[4] = {1, 0, 1, -1}, kDy[4] = {0, 1, 1, 1};

}  // namespace

template <uint32_t MASK, uint32_t PIX>
__global__ __launch_bounds__(kProjThreads) void pairs_kernel(PairsParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    static_assert(MASK == 1u || MASK == 3u || MASK == 15u, "the three instances");
    constexpr uint32_t G = kPairsGroup, kTiles = kProjTilesOf(PIX), kDmax = 8u * PIX, kNpx = 8u / PIX;   // kNpx: pixels per lane
    constexpr uint32_t kBits = 8u * PIX, kPxMask = (1u << kBits) - 1u;
    constexpr uint32_t HL = kPairsHaloLeft(MASK), HR = kPairsHaloRight(MASK), S = kPairsStrideOf(MASK, PIX);
    constexpr bool kBelow = (MASK & ~kPairRight) != 0u;          // an offset with dy = 1: the row below is needed
    constexpr uint32_t NR = kBelow ? 2u : 1u;                    // prefixes: the piece's tile row, the tile row below
    constexpr uint32_t NB = popc(MASK), kRows = kPairsBandRowsOf(MASK), kRowDw = kPairsRowDwords;
    typedef typename std::conditional<PIX == 1u, uint32_t, uint64_t>::type Acc;
    __shared__ uint32_t s_wsum[2][G][NR][2][kProjWaves];   // per group of frames (double-buffered): wave depth totals, sums in front
    __shared__ __attribute__((aligned(8))) uint32_t s_band[2][G][kRows][kRowDw];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // tile of the piece, row of the tile, half of the row (PIX 2)
    const uint32_t t = PIX == 1u ? tid >> 3 : tid >> 4, r = PIX == 1u ? tid & 7u : (tid >> 1) & 7u, hh = PIX == 1u ? 0u : tid & 1u;
    const uint32_t slot = PIX == 1u ? t : 2u * t + hh;   // the lane's two dwords of a band row: 2 + 2 * slot
    const uint32_t per_seg = p.rows * p.pieces;
    const uint32_t seg = blockIdx.x / per_seg;
    const uint32_t rem = blockIdx.x - seg * per_seg;
    const uint32_t br = rem / p.pieces, pc = rem - br * p.pieces;
    const uint32_t ty = p.ty0 + br, txp = p.tx0 + pc * S;
    const uint32_t tx_b = (uint32_t)(p.x0 + p.rw - 1) >> 3;
    const uint32_t nt = tx_b + 1u - txp < kTiles ? tx_b + 1u - txp : kTiles;   // >= 1 (kPairsPiecesOf)
    const bool has_tile = t < nt;
    const bool below = kBelow && br + 1u < p.rows;     // the window has a tile row under this one
    const uint32_t cstride = p.geom.cpf + 1u;
    // the first tile (stream order) of the piece and of the row below, its chunk, that chunk's first tile
    uint32_t pos0[NR], ch[NR], cb[NR], npre[NR];
#pragma unroll
    for (uint32_t rr = 0; rr < NR; rr++) {
        pos0[rr] = (ty + (rr && below ? 1u : 0u)) * p.w + txp;
        ch[rr] = dec_chunk_of(p.geom, pos0[rr]);
        cb[rr] = dec_chunk_begin(p.geom, ch[rr]);
        npre[rr] = pos0[rr] - cb[rr];                  // < 512 (roi_index_geometry)
    }
    const uint32_t f_begin = seg * p.fps;
    const uint64_t f_last = (uint64_t)f_begin + p.fps;
    const uint32_t f_end = f_last < p.n_frames ? (uint32_t)f_last : p.n_frames;
    const uint8_t *const end = p.stream + p.stream_bytes;

    // ---- this lane's pixels in the window and the sums ----
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const int yy = 8 * (int)ty + (int)r;
    const int xx0 = 8 * (int)(txp + t) + 4 * (int)hh;                  // the lane's first pixel column
    const bool owned = has_tile && (pc == 0u || t >= HL) && (pc + 1u == p.pieces || t < kTiles - HR);
    const bool row_in = owned && yy >= p.y0 && yy < p.y0 + p.rh;
    const uint64_t row0 = row_in ? (uint64_t)(yy - p.y0) * (uint64_t)p.rw : 0u;

    Acc acc[NB][kNpx];
#pragma unroll
    for (uint32_t j = 0; j < NB; j++)
#pragma unroll
        for (uint32_t i = 0; i < kNpx; i++) acc[j][i] = 0u;

    // ---- the per-frame words of a group: lane k < G holds frame g0 + k ----
    struct Words {
        uint32_t ok, base[NR];
        uint64_t fo;
    };
    auto issue_words = [&](Words &wd, uint32_t g0) __attribute__((always_inline)) {
        const uint32_t g = g0 + (lane < G ? lane : 0u);
        wd.ok = 0u; wd.fo = 0u;
#pragma unroll
        for (uint32_t rr = 0; rr < NR; rr++) wd.base[rr] = 0u;
        if (lane < G && g < f_end) {
            wd.ok = p.frame_ok[g];
            wd.fo = p.frame_offsets[g];
#pragma unroll
            for (uint32_t rr = 0; rr < NR; rr++) wd.base[rr] = p.chunk_off[(size_t)g * cstride + ch[rr]];
        }
    };

    // ---- one group of frames in flight ----
    struct Meta {
        uint32_t ok[G];                // uniform: frame accepted (and inside the segment)
        const uint8_t *fb[G];          // uniform: the frame
        uint32_t base[NR][G];          // uniform: payload words of the frame in front of the row's chunk
        uint32_t d8[NR][G], ml[NR][G], mh[NR][G];   // depth, minimum (PIX 2: its low / high byte) of this lane's tile (raw loads)
        uint32_t pre[NR][G];           // this lane's dword of the depth bytes in front of the row's first tile (masked where used)
    };
    struct Pay {
        uint32_t a0[NR][G], a1[NR][G], a2[NR][G];   // the aligned dwords around this lane's (half) row
        uint32_t dms[NR][G];                        // PIX 1: depth | minimum << 8 | byte shift << 16; PIX 2: depth | shift << 8 | minimum << 16
    };

    // pre: depth bytes [cb, pos0) of the frame, as aligned dwords, lane tid < ndw holding dword tid.  Every load is
    // unconditional inside an accepted frame (lanes without a tile read tile 0, lanes past ndw dword 0) and nothing
    // consumes a loaded value here, so that the loads stay in flight while the group in front is multiplied.
    // The U16 minima start at 28 + T, possibly at an odd address: read byte by byte.
    auto issue_meta = [&](Meta &m, const Words &wd) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            m.ok[k] = 0u; m.fb[k] = p.stream;
#pragma unroll
            for (uint32_t rr = 0; rr < NR; rr++) { m.base[rr][k] = 0u; m.d8[rr][k] = 0u; m.ml[rr][k] = 0u; m.mh[rr][k] = 0u; m.pre[rr][k] = 0u; }
            m.ok[k] = readlane(wd.ok, k);   // 0 past the segment
            if (m.ok[k]) {
                const uint64_t fo = (uint64_t)readlane((uint32_t)wd.fo, k) | ((uint64_t)readlane((uint32_t)(wd.fo >> 32), k) << 32);
                m.fb[k] = p.stream + fo;   // validated: the whole frame lies inside stream_bytes
                const uint8_t *darr = m.fb[k] + 24;
                const uint32_t tt = has_tile ? t : 0u;
#pragma unroll
                for (uint32_t rr = 0; rr < NR; rr++) {
                    if (rr && !below) continue;
                    m.base[rr][k] = readlane(wd.base[rr], k);
                    m.d8[rr][k] = darr[pos0[rr] + tt];
                    if constexpr (PIX == 1u) {
                        m.ml[rr][k] = darr[4u + p.T + pos0[rr] + tt];
                    } else {
                        m.ml[rr][k] = darr[4u + p.T + 2u * (pos0[rr] + tt)];
                        m.mh[rr][k] = darr[5u + p.T + 2u * (pos0[rr] + tt)];
                    }
                    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(darr + cb[rr]) & 3u), ndw = (head + npre[rr] + 3u) >> 2;
                    const uint8_t *a_lo = darr + cb[rr] - head;   // (pointer arithmetic: the load stays a global one)
                    m.pre[rr][k] = *reinterpret_cast<const uint32_t *>(a_lo + 4u * (tid < ndw ? tid : 0u));   // inside the frame
                }
            }
        }
    };
    // the group's tile offsets (the group's one barrier, which also publishes the band written in front of it) and its
    // payload loads.  In the row below only the lanes of tile row 0 load: its row 0 is all that is needed.
    uint32_t buf = 0;
    auto issue_payload = [&](const Meta &m, Pay &q) __attribute__((always_inline)) {
        uint32_t any = 0;
#pragma unroll
        for (uint32_t k = 0; k < G; k++) any |= m.ok[k];
#pragma unroll
        for (uint32_t rr = 0; rr < NR; rr++)
#pragma unroll
            for (uint32_t k = 0; k < G; k++) { q.a0[rr][k] = q.a1[rr][k] = q.a2[rr][k] = 0u; q.dms[rr][k] = 0u; }
        if (!any) {
            __syncthreads();
            return;
        }
        uint32_t incl[NR][G];
#pragma unroll
        for (uint32_t rr = 0; rr < NR; rr++) {
            if (rr && !below) continue;
#pragma unroll
            for (uint32_t k = 0; k < G; k++) {
                const uint32_t d = has_tile ? (m.d8[rr][k] > kDmax ? kDmax : m.d8[rr][k]) : 0u;   // (a validated frame has none above)
                incl[rr][k] = wave_scan_incl((PIX == 1u ? r == 0u : (tid & 15u) == 0u) ? d : 0u);   // the tile's first lane
                const uint32_t pw = wave_sum(__builtin_amdgcn_sad_u8(m.pre[rr][k] & pre_keep(m.fb[k], cb[rr], npre[rr], tid), 0u, 0u));
                if (lane == 63u) s_wsum[buf][k][rr][0][wave] = incl[rr][k];
                if (lane == 0u) s_wsum[buf][k][rr][1][wave] = pw;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t rr = 0; rr < NR; rr++) {
            if (rr && !below) continue;
#pragma unroll
            for (uint32_t k = 0; k < G; k++) {
                uint32_t wbase = 0, PRE = 0;
#pragma unroll
                for (uint32_t w = 0; w < kProjWaves; w++) {
                    wbase += w < wave ? s_wsum[buf][k][rr][0][w] : 0u;
                    PRE += s_wsum[buf][k][rr][1][w];
                }
                const uint32_t d = has_tile ? (m.d8[rr][k] > kDmax ? kDmax : m.d8[rr][k]) : 0u;
                const uint32_t woff = m.base[rr][k] + PRE + wbase + incl[rr][k] - d;   // payload words in front of the tile
                const uint32_t rw_ = rr ? 0u : r;                                      // the tile row this lane loads
                // PIX 2, the half row: byte r * d + h * (d / 2), a nibble further when d is odd; 4d bits (+ 4) <= 8 bytes
                const uint8_t *src = m.fb[k] + 32 + (PIX + 1ull) * p.T + 8ull * woff + rw_ * d + hh * (d >> 1);
                const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
                const uint8_t *q8 = src - sh;   // (pointer arithmetic: the loads stay global ones)
                const bool need = m.ok[k] && has_tile && d != 0u && (rr == 0u || r == 0u), tail = q8 + 12 > end;
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
                q.a0[rr][k] = w0; q.a1[rr][k] = w1; q.a2[rr][k] = w2;
                q.dms[rr][k] = pack_dms<PIX>(d, sh, m.ml[rr][k], m.mh[rr][k]);
            }
        }
        buf ^= 1u;
    };

    // the lane's (half) row of frame k of prefix rr: two dwords of four U8 or two U16 pixels each
    auto decode = [&](const Pay &q, uint32_t rr, uint32_t k, uint32_t &v0, uint32_t &v1) __attribute__((always_inline)) {
        cut_row<PIX>(q.a0[rr][k], q.a1[rr][k], q.a2[rr][k], q.dms[rr][k], hh, v0, v1);
    };

    // the group's rows -> the band (in front of the group's barrier)
    uint32_t bb = 0;
    auto stage = [&](const Meta &m, const Pay &q) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!m.ok[k]) continue;   // rejected (or past the segment): adds nothing
            uint32_t v0, v1;
            decode(q, 0u, k, v0, v1);
            *reinterpret_cast<uint2 *>(&s_band[bb][k][r][2u + 2u * slot]) = make_uint2(v0, v1);
            if constexpr (kBelow) {
                if (below && r == 0u) {
                    decode(q, 1u, k, v0, v1);
                    *reinterpret_cast<uint2 *>(&s_band[bb][k][8][2u + 2u * slot]) = make_uint2(v0, v1);
                }
            }
        }
    };
    // pixel i of the two dwords v0, v1
    auto px_of = [&](uint32_t v0, uint32_t v1, uint32_t i) __attribute__((always_inline)) -> uint32_t {
        constexpr uint32_t kPerDw = 4u / PIX;
        return ((i < kPerDw ? v0 : v1) >> (kBits * (i % kPerDw))) & kPxMask;
    };
    // the band (behind the group's barrier) -> the sums
    auto consume = [&](const Meta &m) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!m.ok[k]) continue;
            const uint32_t *const row = &s_band[bb][k][r][2u + 2u * slot];
            const uint2 own = *reinterpret_cast<const uint2 *>(row);
            uint32_t a[kNpx], b[kNpx + 2u];   // own pixels; the row below from one pixel to the left to one to the right
#pragma unroll
            for (uint32_t i = 0; i < kNpx; i++) a[i] = px_of(own.x, own.y, i);
            uint32_t j = 0;
            if constexpr ((MASK & kPairRight) != 0u) {
                const uint32_t an = row[2] & kPxMask;
#pragma unroll
                for (uint32_t i = 0; i < kNpx; i++) acc[j][i] += (Acc)a[i] * (Acc)(i + 1u < kNpx ? a[i + 1u] : an);
                j++;
            }
            if constexpr (kBelow) {
                const uint32_t *const rb = row + kRowDw;   // row r + 1; band row 8 is row 0 of the tile row below
                const uint32_t bl = rb[-1], bn = rb[2];
                const uint2 bo = *reinterpret_cast<const uint2 *>(rb);
                b[0] = bl >> (32u - kBits);
#pragma unroll
                for (uint32_t i = 0; i < kNpx; i++) b[1u + i] = px_of(bo.x, bo.y, i);
                b[kNpx + 1u] = bn & kPxMask;
                if constexpr ((MASK & kPairDown) != 0u) {
#pragma unroll
                    for (uint32_t i = 0; i < kNpx; i++) acc[j][i] += (Acc)a[i] * (Acc)b[1u + i];
                    j++;
                }
                if constexpr ((MASK & kPairDownRight) != 0u) {
#pragma unroll
                    for (uint32_t i = 0; i < kNpx; i++) acc[j][i] += (Acc)a[i] * (Acc)b[2u + i];
                    j++;
                }
                if constexpr ((MASK & kPairDownLeft) != 0u) {
#pragma unroll
                    for (uint32_t i = 0; i < kNpx; i++) acc[j][i] += (Acc)a[i] * (Acc)b[i];
                    j++;
                }
            }
        }
        bb ^= 1u;
    };

    // ---- the pipeline: multiply group k while group k + 1's payload and group k + 2's depth bytes load ----
    Meta m_cur, m_nxt, m_nn;
    Pay q_cur, q_nxt;
    Words w_nn;
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

    // ---- the owned window pixels of this lane -> the requested planes, or this segment's partials ----
    if (row_in) {
        const bool direct = p.segments == 1u;
#pragma unroll
        for (uint32_t i = 0; i < kNpx; i++) {
            const int xx = xx0 + (int)i;
            if (xx < p.x0 || xx >= p.x0 + p.rw) continue;
            const uint64_t o = row0 + (uint64_t)(xx - p.x0);
            uint32_t j = 0, plane = 0;
#pragma unroll
            for (uint32_t bit = 0; bit < 4u; bit++) {
                if (!((MASK >> bit) & 1u)) continue;
                const Acc v = acc[j++][i];
                if (!((p.pairs >> bit) & 1u)) continue;
                const int px = xx + kDx[bit], py = yy + kDy[bit];
                const bool partner = px >= p.x0 && px < p.x0 + p.rw && py < p.y0 + p.rh;
                const uint64_t at = (uint64_t)plane * P + o;
                plane++;
                if (direct) {
                    if (partner) p.out[at] = p.accumulate ? p.out[at] + v : (uint64_t)v;
                    else if (!p.accumulate) p.out[at] = 0u;
                } else {
                    static_cast<Acc *>(p.ws)[(uint64_t)seg * p.planes * P + at] = partner ? v : (Acc)0u;
                }
            }
        }
    }
    if (p.segments == 1u && blockIdx.x == 0u) write_count(p);
}

// Segments > 1: prior (ACC: what the planes hold) + partial 0 + partial 1 + ..., exact U64 additions.  One thread per
// window pixel, looping over the planes; the partials are [segments][planes][rw * rh], so each read is coalesced.
template <typename Part, bool ACC>
__global__ __launch_bounds__(kProjCombineThreads) void pairs_combine_kernel(PairsParams p) {
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const uint64_t i = (uint64_t)blockIdx.x * kProjCombineThreads + threadIdx.x;
    if (i < P) {
        const uint64_t KP = (uint64_t)p.planes * P;
        for (uint32_t j = 0; j < p.planes; j++) {
            const Part *const ws = static_cast<const Part *>(p.ws) + (uint64_t)j * P + i;
            uint64_t *const out = p.out + (uint64_t)j * P + i;
            uint64_t v = ACC ? *out : 0u;
            for (uint32_t s = 0; s < p.segments; s++) v += ws[(uint64_t)s * KP];
            *out = v;
        }
    }
    if (blockIdx.x == 0u) write_count(p);
}

uint64_t pairs_workspace_bytes(uint32_t planes, uint32_t segments, uint64_t pixels, uint32_t pix) {
    if (segments <= 1u) return 0;
    return (4ull * pix * segments * planes * pixels + 15u) & ~(uint64_t)15;
}

typedef void (*PairsKernel)(PairsParams);

hipError_t launch_pairs(const PairsParams &p, uint32_t pix, hipStream_t s) {
    if (p.pairs < 1u || p.pairs > kPairAll || p.planes != popc(p.pairs) || (pix != 1u && pix != 2u)) return hipErrorInvalidValue;
    const uint32_t inst = kPairsInstanceOf(p.pairs);
    PairsKernel k;
    if (pix == 1u) k = inst == 1u ? pairs_kernel<1, 1> : inst == 3u ? pairs_kernel<3, 1> : pairs_kernel<15, 1>;
    else k = inst == 1u ? pairs_kernel<1, 2> : inst == 3u ? pairs_kernel<3, 2> : pairs_kernel<15, 2>;
    const uint32_t grid = p.pieces * p.rows * p.segments;   // (the host keeps it below 2^31)
    hipLaunchKernelGGL(k, dim3(grid), dim3(kProjThreads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.segments == 1u) return e;
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const uint32_t cgrid = (uint32_t)((P + kProjCombineThreads - 1u) / kProjCombineThreads);
    PairsKernel combine;
    if (pix == 1u) combine = p.accumulate ? pairs_combine_kernel<uint32_t, true> : pairs_combine_kernel<uint32_t, false>;
    else combine = p.accumulate ? pairs_combine_kernel<uint64_t, true> : pairs_combine_kernel<uint64_t, false>;
    hipLaunchKernelGGL(combine, dim3(cgrid), dim3(kProjCombineThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
