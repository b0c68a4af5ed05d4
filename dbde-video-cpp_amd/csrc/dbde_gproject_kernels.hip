// dbde_gproject_kernels.hip -- grouped temporal projections for MI355X (gfx950, wave64): per-pixel maximum, minimum, sum
// and sum of squares of the rw x rh window over every GROUP of frames of a batch, one set of planes per group, straight
// from the compressed bytes (no image is written).  DESIGN.md 4.14.
//
// gproject_kernel<STATS, PIX> is project_kernel's walk (dbde_project_kernels.hip: the same lane mapping, 8 * PIX lanes per
// tile, the same expand_row / add_bytes / cut_four16 cuts, the same DPP offsets scan and three-deep load pipeline) with
// the frames of a workgroup taken from a list of SLOTS instead of a range:
//   a workgroup owns one window tile row, one piece of kProjTilesOf(PIX) tiles and a run of consecutive groups
//   [k_begin, k_end).  The run's slots are, group by group, the group's frames [b, e) in order, the last one flagged
//   "flush"; an empty group is one slot without a frame, flagged "flush".  Slots past the run's last are padding.
// The words stage walks a uniform cursor (group, next frame, group end) through the slots, four to a pipeline step, so
// a step may hold the last frames of one group and the first of the next, wherever the next group begins: the pipeline
// never drains at a group boundary, in the uniform form (groups of group_frames frames) and in the ragged one (groups
// from group_starts, clamped here: b = min(s[k], n), e = min(max(s[k + 1], s[k]), n)).
// After a slot flagged "flush" has been folded in, the lane writes its pixels of the window into group k's planes
// (converted to the planes' types, a lane wholly inside the window in one store per statistic; read-combine-write,
// pixel by pixel, when accumulating) and resets its accumulators.  The stores are not waited for.  The run's first workgroup (tile row 0, piece 0) also writes the group's count of accepted frames.
// Every value is an exact integer: a group holds at most kGProjMaxGroupFrames frames (U32 sums, U32 sums of squares of
// U8 pixels; U64 sums of squares of U16 pixels).
#include "dbde_gproject_kernels.h"

#include <type_traits>
#include <utility>

#include "dbde_proj_pipeline.h"

namespace dbde {

namespace {

constexpr uint32_t kGProjStep = 4;                 // slots per pipeline step

template <uint32_t PIX> using GProjPix = typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type;
template <uint32_t PIX> using GProjSq = typename std::conditional<PIX == 1u, uint32_t, uint64_t>::type;

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

}  // namespace

template <uint32_t STATS, uint32_t PIX>
__global__ __launch_bounds__(kProjThreads) void gproject_kernel(GProjParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    typedef GProjPix<PIX> Pix;
    constexpr bool kMax = (STATS & kProjMax) != 0u, kMin = (STATS & kProjMin) != 0u;
    constexpr bool kSum = (STATS & kProjSum) != 0u, kSq = (STATS & kProjSumSq) != 0u;
    constexpr uint32_t G = kGProjStep, kTiles = kProjTilesOf(PIX), kDmax = 8u * PIX, kNpx = 8u / PIX;   // kNpx: pixels per lane
    constexpr uint32_t kPixMask = PIX == 1u ? 0xFFu : 0xFFFFu;
    __shared__ uint32_t s_wsum[2][G][2][kProjWaves];   // per step (double-buffered): wave depth totals, sums in front

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // tile of the piece, row of the tile, half of the row (PIX 2)
    const uint32_t t = PIX == 1u ? tid >> 3 : tid >> 4, r = PIX == 1u ? tid & 7u : (tid >> 1) & 7u, hh = PIX == 1u ? 0u : tid & 1u;
    const uint32_t per_run = p.rows * p.pieces;
    const uint32_t run = blockIdx.x / per_run;
    const uint32_t rem = blockIdx.x - run * per_run;
    const uint32_t br = rem / p.pieces, pc = rem - br * p.pieces;
    const uint32_t ty = p.ty0 + br, txp = p.tx0 + pc * kTiles;
    const uint32_t tx_b = (uint32_t)(p.x0 + p.rw - 1) >> 3;
    const uint32_t nt = tx_b + 1u - txp < kTiles ? tx_b + 1u - txp : kTiles;
    const bool has_tile = t < nt;
    const uint32_t pos0 = ty * p.w + txp;              // the piece's first tile (stream order)
    const uint32_t c = dec_chunk_of(p.geom, pos0), cb = dec_chunk_begin(p.geom, c);
    const uint32_t npre = pos0 - cb;                   // < 512 (roi_index_geometry)
    const uint32_t cstride = p.geom.cpf + 1u;
    const uint32_t k_begin = run * p.gpr;              // (runs * gpr < n_groups + gpr: no overflow, the host checks)
    const uint32_t k_end = p.n_groups - k_begin < p.gpr ? p.n_groups : k_begin + p.gpr;
    const uint8_t *const end = p.stream + p.stream_bytes;

    // ---- accumulators: this lane's kNpx pixels of the current group ----
    // max / min: PIX 1 even bytes (mx, mn) and odd bytes (mxo, mno) of pixels 0-3, 4-7; PIX 2 U16 pairs (mx, mn)
    uint32_t mx[2] = {0u, 0u}, mxo[2] = {0u, 0u};
    uint32_t mn[2] = {~0u, ~0u}, mno[2] = {~0u, ~0u};
    uint32_t sum[kNpx] = {};
    GProjSq<PIX> sq[kNpx] = {};

    // ---- the slot cursor of the words stage (uniform): group kw, its next frame fw and its end ew ----
    auto group_range = [&](uint32_t k, uint32_t &b, uint32_t &e) __attribute__((always_inline)) {
        if (p.group_starts) {   // clamped, never trusted
            const uint32_t s0 = p.group_starts[k], s1 = p.group_starts[k + 1u];
            b = s0 < p.n_frames ? s0 : p.n_frames;
            const uint32_t hi = s1 > s0 ? s1 : s0;
            e = hi < p.n_frames ? hi : p.n_frames;
        } else {                // k * group_frames < n_frames (n_groups = ceil(n_frames / group_frames))
            b = k * p.group_frames;
            e = p.n_frames - b < p.group_frames ? p.n_frames : b + p.group_frames;
        }
    };
    uint32_t kw = k_begin, fw = 0u, ew = 0u;
    if (kw < k_end) group_range(kw, fw, ew);

    // ---- the per-frame words of a step, one step ahead of their use: lane k < G holds slot k's frame ----
    struct Words {
        uint32_t ok, base;
        uint64_t fo;
        uint32_t fl;               // uniform: bit k = slot k ends its group
    };
    auto issue_words = [&](Words &wd) __attribute__((always_inline)) {
        uint32_t fsel = 0u, fl = 0u;
        bool mine = false;
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (kw < k_end) {
                if (fw < ew) {
                    if (lane == k) { fsel = fw; mine = true; }
                    fw++;
                }
                if (fw >= ew) {   // the group's last frame (or an empty group): flush after this slot, on to the next group
                    fl |= 1u << k;
                    kw++;
                    if (kw < k_end) group_range(kw, fw, ew);
                    fw = uniform(fw);
                    ew = uniform(ew);
                }
            }
        }
        wd.ok = 0u; wd.base = 0u; wd.fo = 0u;
        wd.fl = fl;
        if (mine) {   // fsel < ew <= n_frames
            wd.ok = p.frame_ok[fsel];
            wd.fo = p.frame_offsets[fsel];
            wd.base = p.chunk_off[(size_t)fsel * cstride + c];
        }
    };

    // ---- one step of slots in flight ----
    struct Meta {
        uint32_t ok[G];            // uniform: the slot has an accepted frame
        uint32_t fl;               // uniform: the slots that end their group
        uint32_t base[G];          // uniform: payload words of the frame in front of the piece's chunk
        const uint8_t *fb[G];      // uniform: the frame
        uint32_t d8[G], ml[G], mh[G];   // depth, minimum (PIX 2: its low / high byte) of this lane's tile (raw loads)
        uint32_t pre[G];           // this lane's dword of the depth bytes in front of the piece (masked where used)
    };
    struct Pay {
        uint32_t a0[G], a1[G], a2[G];   // the aligned dwords around this lane's (half) row
        uint32_t dms[G];                // PIX 1: depth | minimum << 8 | byte shift << 16; PIX 2: depth | shift << 8 | minimum << 16
    };

    // (project_kernel's issue_meta: every load unconditional inside an accepted frame, none consumed here)
    auto issue_meta = [&](Meta &m, const Words &wd) __attribute__((always_inline)) {
        m.fl = wd.fl;
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            m.ok[k] = 0u; m.base[k] = 0u; m.fb[k] = p.stream; m.d8[k] = 0u; m.ml[k] = 0u; m.pre[k] = 0u;
            if constexpr (PIX == 2u) m.mh[k] = 0u;
            m.ok[k] = readlane(wd.ok, k);   // 0 for a slot without a frame
            if (m.ok[k]) {
                const uint64_t fo = (uint64_t)readlane((uint32_t)wd.fo, k) | ((uint64_t)readlane((uint32_t)(wd.fo >> 32), k) << 32);
                m.fb[k] = p.stream + fo;   // validated: the whole frame lies inside stream_bytes
                m.base[k] = readlane(wd.base, k);
                const uint8_t *darr = m.fb[k] + 24;
                const uint32_t tt = has_tile ? t : 0u;
                m.d8[k] = darr[pos0 + tt];
                if constexpr (PIX == 1u) {
                    m.ml[k] = darr[4u + p.T + pos0 + tt];
                } else {
                    m.ml[k] = darr[4u + p.T + 2u * (pos0 + tt)];
                    m.mh[k] = darr[5u + p.T + 2u * (pos0 + tt)];
                }
                const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(darr + cb) & 3u), ndw = (head + npre + 3u) >> 2;
                const uint8_t *a_lo = darr + cb - head;   // (pointer arithmetic: the load stays a global one)
                m.pre[k] = *reinterpret_cast<const uint32_t *>(a_lo + 4u * (tid < ndw ? tid : 0u));   // inside the frame
            }
        }
    };
    // the step's tile offsets (one barrier) and its payload loads
    uint32_t buf = 0;
    auto issue_payload = [&](const Meta &m, Pay &q) __attribute__((always_inline)) {
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
            const uint32_t d = has_tile ? (m.d8[k] > kDmax ? kDmax : m.d8[k]) : 0u;   // (a validated frame has none above)
            incl[k] = wave_scan_incl((PIX == 1u ? r == 0u : (tid & 15u) == 0u) ? d : 0u);   // the tile's first lane
            const uint32_t pw = wave_sum(__builtin_amdgcn_sad_u8(m.pre[k] & pre_keep(m.fb[k], cb, npre, tid), 0u, 0u));
            if (lane == 63u) s_wsum[buf][k][0][wave] = incl[k];
            if (lane == 0u) s_wsum[buf][k][1][wave] = pw;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            uint32_t wbase = 0, PRE = 0;
#pragma unroll
            for (uint32_t w = 0; w < kProjWaves; w++) {
                wbase += w < wave ? s_wsum[buf][k][0][w] : 0u;
                PRE += s_wsum[buf][k][1][w];
            }
            const uint32_t d = has_tile ? (m.d8[k] > kDmax ? kDmax : m.d8[k]) : 0u;
            const uint32_t woff = m.base[k] + PRE + wbase + incl[k] - d;   // payload words in front of the tile
            // PIX 2, the half row: byte r * d + h * (d / 2), a nibble further when d is odd; 4d bits (+ 4) <= 8 bytes
            const uint8_t *src = m.fb[k] + 32 + (PIX + 1ull) * p.T + 8ull * woff + r * d + hh * (d >> 1);
            const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
            const uint8_t *q8 = src - sh;   // (pointer arithmetic: the loads stay global ones)
            const bool need = m.ok[k] && has_tile && d != 0u, tail = q8 + 12 > end;
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

    // ---- this lane's pixels of the window -> group k's planes; the accumulators start again ----
    // Where the lane's pixels go is worked out at the flush, from a lane id the compiler cannot see through: hoisted out
    // of the loop these values would hold VGPRs for the whole walk and cost a wave of occupancy.
    Pix *const out_max = reinterpret_cast<Pix *>(p.out_max), *const out_min = reinterpret_cast<Pix *>(p.out_min);
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    uint32_t kc = k_begin, cnt = 0u;   // uniform: the group being accumulated, its accepted frames so far
    auto flush = [&]() __attribute__((always_inline)) {
        uint32_t tq = tid;
        asm volatile("" : "+v"(tq));
        const uint32_t t = PIX == 1u ? tq >> 3 : tq >> 4, r = PIX == 1u ? tq & 7u : (tq >> 1) & 7u, hh = PIX == 1u ? 0u : tq & 1u;
        const int yy = 8 * (int)ty + (int)r;
        const bool in_rows = t < nt && yy >= p.y0 && yy < p.y0 + p.rh;
        const uint64_t row0 = (uint64_t)(yy - p.y0) * (uint64_t)p.rw;
        // a lane whose kNpx pixels all lie inside the window stores each statistic in one piece (the planes' natural
        // alignment only: the runtime's unaligned access mode carries a U8 plane at an odd address)
        const int xx0 = 8 * (int)(txp + t) + 4 * (int)hh;
        const bool whole = xx0 >= p.x0 && xx0 + (int)kNpx <= p.x0 + p.rw && !p.accumulate;
        if (in_rows && whole) {
            const uint64_t o = (uint64_t)kc * P + row0 + (uint64_t)(xx0 - p.x0);
            if (kMax) {   // PIX 1: even bytes from mx, odd bytes from the high bytes of mxo's 16-bit lanes
                const uint32_t v[2] = {PIX == 1u ? (mx[0] & 0x00FF00FFu) | (mxo[0] & 0xFF00FF00u) : mx[0],
                                       PIX == 1u ? (mx[1] & 0x00FF00FFu) | (mxo[1] & 0xFF00FF00u) : mx[1]};
                __builtin_memcpy(out_max + o, v, 8);
            }
            if (kMin) {
                const uint32_t v[2] = {PIX == 1u ? (mn[0] & 0x00FF00FFu) | (mno[0] & 0xFF00FF00u) : mn[0],
                                       PIX == 1u ? (mn[1] & 0x00FF00FFu) | (mno[1] & 0xFF00FF00u) : mn[1]};
                __builtin_memcpy(out_min + o, v, 8);
            }
            if (kSum) {
                if (PIX == 1u && p.sum16) {
                    uint32_t v[kNpx / 2u];
#pragma unroll
                    for (int i = 0; i < (int)kNpx / 2; i++) v[i] = (sum[2 * i] & 0xFFFFu) | (sum[2 * i + 1] << 16);
                    __builtin_memcpy(static_cast<uint16_t *>(p.out_sum) + o, v, 2u * kNpx);
                } else {
                    __builtin_memcpy(static_cast<uint32_t *>(p.out_sum) + o, sum, 4u * kNpx);
                }
            }
            if (kSq) {
                uint64_t v[kNpx];
#pragma unroll
                for (int i = 0; i < (int)kNpx; i++) v[i] = sq[i];
                __builtin_memcpy(p.out_sumsq + o, v, 8u * kNpx);
            }
        } else if (in_rows) {
            const uint64_t g0 = (uint64_t)kc * P + row0;
#pragma unroll
            for (int i = 0; i < (int)kNpx; i++) {
                const int xx = 8 * (int)(txp + t) + 4 * (int)hh + i;
                if (xx < p.x0 || xx >= p.x0 + p.rw) continue;
                const uint64_t o = g0 + (uint64_t)(xx - p.x0);
                // pixel i of a packed max / min: PIX 1 byte i & 3 of the even / odd accumulator, PIX 2 U16 i & 1 of a pair
                const int h = PIX == 1u ? i >> 2 : i >> 1, sb = PIX == 1u ? 8 * (i & 3) : 16 * (i & 1);
                if (kMax) {
                    uint32_t v = ((PIX == 1u && (i & 1)) ? mxo[h] : mx[h]) >> sb & kPixMask;
                    if (p.accumulate) { const uint32_t ov = out_max[o]; v = v > ov ? v : ov; }
                    out_max[o] = (Pix)v;
                }
                if (kMin) {
                    uint32_t v = ((PIX == 1u && (i & 1)) ? mno[h] : mn[h]) >> sb & kPixMask;
                    if (p.accumulate) { const uint32_t ov = out_min[o]; v = v < ov ? v : ov; }
                    out_min[o] = (Pix)v;
                }
                if (kSum) {
                    if (PIX == 1u && p.sum16) {   // (never with accumulate: the host refuses it)
                        static_cast<uint16_t *>(p.out_sum)[o] = (uint16_t)sum[i];
                    } else {
                        uint32_t *const os = static_cast<uint32_t *>(p.out_sum);
                        os[o] = (p.accumulate ? os[o] : 0u) + sum[i];
                    }
                }
                if (kSq) p.out_sumsq[o] = (p.accumulate ? p.out_sumsq[o] : 0ull) + sq[i];
            }
        }
        if (rem == 0u && tid == 0u) p.out_counts[kc] = (p.accumulate ? p.out_counts[kc] : 0u) + cnt;
#pragma unroll
        for (int h = 0; h < 2; h++) { mx[h] = 0u; mxo[h] = 0u; mn[h] = ~0u; mno[h] = ~0u; }
#pragma unroll
        for (int i = 0; i < (int)kNpx; i++) { sum[i] = 0u; sq[i] = 0; }
        kc++;
        cnt = 0u;
    };

    auto accumulate = [&](const Meta &m, const Pay &q) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (m.ok[k]) {   // (a rejected frame, an empty group's slot or padding contributes nothing)
                cnt++;
                uint32_t px[2];
                cut_row<PIX>(q.a0[k], q.a1[k], q.a2[k], q.dms[k], hh, px[0], px[1]);
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
            if ((m.fl >> k) & 1u) flush();
        }
    };

    // ---- the pipeline: accumulate step s while step s + 1's payload and step s + 2's depth bytes load ----
    Meta m_cur, m_nxt, m_nn;
    Pay q_cur, q_nxt;
    Words w_nn;
    issue_words(w_nn);
    issue_meta(m_cur, w_nn);
    issue_payload(m_cur, q_cur);
    issue_words(w_nn);
    issue_meta(m_nxt, w_nn);
    issue_words(w_nn);
    while (kc < k_end) {   // (every step in front of the run's last flush holds a frame or ends a group)
        issue_payload(m_nxt, q_nxt);
        issue_meta(m_nn, w_nn);
        issue_words(w_nn);
        accumulate(m_cur, q_cur);
        m_cur = m_nxt;
        q_cur = q_nxt;
        m_nxt = m_nn;
    }
}

typedef void (*GProjKernel)(GProjParams);
struct GProjTable {
    GProjKernel k[16];   // [stats]: gproject_kernel<stats, PIX>, 1..15
};

template <uint32_t PIX, uint32_t... S>
static constexpr GProjTable gproj_table(std::integer_sequence<uint32_t, S...>) {
    return {{nullptr, gproject_kernel<S + 1u, PIX>...}};
}

hipError_t launch_gproject(const GProjParams &p, uint32_t stats, uint32_t pix, hipStream_t s) {
    static const GProjTable tables[2] = {gproj_table<1>(std::make_integer_sequence<uint32_t, 15>()),
                                         gproj_table<2>(std::make_integer_sequence<uint32_t, 15>())};
    if (stats < 1u || stats > kProjAll || (pix != 1u && pix != 2u)) return hipErrorInvalidValue;
    if (p.n_groups == 0u) return hipSuccess;
    const uint32_t grid = p.pieces * p.rows * p.runs;   // (the host keeps it below 2^31)
    hipLaunchKernelGGL(tables[pix - 1u].k[stats], dim3(grid), dim3(kProjThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
