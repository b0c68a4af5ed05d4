// dbde_trace_kernels.hip -- region traces for MI355X (gfx950, wave64): per frame and per labelled region, the maximum,
// minimum, sum and sum of squares of the region's pixels, straight from the compressed bytes (no image is written).
//
// trace_kernel<STATS, PIX>: one workgroup per (frame segment, span), a span being kTraceTilesOf(PIX) consecutive tile
// columns of one tile row that holds at least one active tile of the map (a workgroup of a span without one returns at
// once).  Lanes, loads and the frame pipeline are the projection kernel's (dbde_project_kernels.hip): PIX = 1 one lane
// per tile row (8 pixels, expand_row / add_bytes), PIX = 2 one lane per half tile row (4 U16 pixels, cut_four16); the
// payload offset of a tile comes from its index chunk's offset plus the depth bytes in front of it (the span's depth
// prefix, v_sad_u8, and one DPP scan per wave).  Only active tiles load their minimum and payload; empty tiles give
// their depth byte to the offsets scan and nothing else.
//
// Reduction.  The workgroup's pixels, in lane order (tile, row, half), form one sequence of labels fixed by the map.
// Label-0 pixels are transparent; a run is a maximal stretch of pixels with the same label between them.  Per frame:
//   1. each lane folds its pixels into runs: the first (E), the last (X), and any run between them, which it flushes at
//      once (only a mixed tile row with three or more labels has one);
//   2. a segmented DPP scan over the wave folds the X values of lanes that continue one run (consecutive whole tiles
//      of a label, the rows of one region inside mixed tiles);
//   3. one LDS exchange per group of frames carries runs across the workgroup's four waves;
//   4. the lane where a run ends flushes it: one atomic per requested statistic per (workgroup, frame, run).
// The run structure is the same for every frame, so the lane flags (first / last label, who continues whom, the scan's
// segment heads) are worked out once per workgroup, before the frame loop.
// Statistic values per run and frame: max / min packed as max << 16 | (65,535 - min) (one v_pk_max_u16 folds both), sum
// U32 (at most 2,048 pixels of 255 or 1,024 of 65,535 per workgroup), sum of squares U32 for PIX 1 (2,048 * 255^2 <
// 2^32), U64 for PIX 2.  Sums go to the U64 outputs with global atomics; max / min to the U32 workspace, which
// trace_finish_kernel<PIX> copies into the U8 / U16 outputs.
#include "dbde_trace_kernels.h"

#include <type_traits>
#include <utility>

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

constexpr uint32_t kTraceGroup = 4;                // frames per pipeline step
constexpr uint32_t kTraceWaves = kTraceThreads / 64u;

template <uint32_t PIX> using TracePix = typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type;
template <uint32_t PIX> using TraceSq = typename std::conditional<PIX == 1u, uint32_t, uint64_t>::type;

// The in-kernel U32 sums: one workgroup holds 256 lanes of 8 (PIX 1) or 4 (PIX 2) pixels.
static_assert(256ull * 8u * 255u * 255u < (1ull << 32), "PIX 1: U32 sums of squares of one workgroup");
static_assert(256ull * 4u * 65535u < (1ull << 32), "PIX 2: U32 sums of one workgroup");

__device__ __forceinline__ uint32_t readlane(uint32_t v, uint32_t j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j); }

// Wave-wide inclusive max scan (wave_scan_incl's DPP steps, max instead of add).
__device__ __forceinline__ uint32_t wave_max_incl(uint32_t x) {
    uint32_t t = x, u;
    u = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x111, 0xF, 0xF, false); t = t > u ? t : u;
    u = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x112, 0xF, 0xF, false); t = t > u ? t : u;
    u = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x114, 0xF, 0xF, false); t = t > u ? t : u;
    u = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x118, 0xF, 0xF, false); t = t > u ? t : u;
    u = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x142, 0xA, 0xF, false); t = t > u ? t : u;
    u = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x143, 0xC, 0xF, false); t = t > u ? t : u;
    return t;
}

// One run's statistics (only the requested fields are used).
template <uint32_t PIX> struct Run {
    uint32_t mm;        // max << 16 | (65,535 - min)
    uint32_t s;         // sum
    TraceSq<PIX> q;     // sum of squares
};

// The step of the segmented scan: x is folded with the lane k steps in front when bit `step` of the lane's mask says
// that lane lies in the same run (DPP row_shr 1, 2, 4, 8, then row_bcast 15 and 31, as wave_scan_incl).
template <uint32_t STATS, uint32_t PIX, int CTRL, int ROWS>
__device__ __forceinline__ void scan_step(Run<PIX> &x, bool take) {
    constexpr bool kMM = (STATS & (kProjMax | kProjMin)) != 0u, kSum = (STATS & kProjSum) != 0u, kSq = (STATS & kProjSumSq) != 0u;
    if constexpr (kMM) {
        const uint32_t u = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.mm, CTRL, ROWS, 0xF, false);
        if (take) x.mm = pk_max_u16(x.mm, u);
    }
    if constexpr (kSum) {
        const uint32_t u = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.s, CTRL, ROWS, 0xF, false);
        if (take) x.s += u;
    }
    if constexpr (kSq) {
        if constexpr (PIX == 1u) {
            const uint32_t u = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.q, CTRL, ROWS, 0xF, false);
            if (take) x.q += u;
        } else {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x.q, CTRL, ROWS, 0xF, false);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x.q >> 32), CTRL, ROWS, 0xF, false);
            if (take) x.q += (uint64_t)lo | ((uint64_t)hi << 32);
        }
    }
}

}  // namespace

template <uint32_t STATS, uint32_t PIX>
__global__ __launch_bounds__(kTraceThreads) void trace_kernel(TraceParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    typedef Run<PIX> R;
    constexpr bool kMax = (STATS & kProjMax) != 0u, kMin = (STATS & kProjMin) != 0u;
    constexpr bool kSum = (STATS & kProjSum) != 0u, kSq = (STATS & kProjSumSq) != 0u;
    constexpr uint32_t G = kTraceGroup, kTiles = kTraceTilesOf(PIX), kDmax = 8u * PIX, kNpx = 8u / PIX;   // kNpx: pixels per lane
    __shared__ uint32_t s_wsum[2][G][2][kTraceWaves];   // per group of frames (double-buffered): wave depth totals, sums in front
    __shared__ uint32_t s_tail[2][G][kTraceWaves][4];   // per group of frames (double-buffered): each wave's last lane's run
    __shared__ uint32_t s_kind[kTiles];                 // the span's tile words (0: empty)
    __shared__ uint32_t s_wmax[kTraceWaves], s_whole[kTraceWaves], s_l0cont[kTraceWaves];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // tile of the span, row of the tile, half of the row (PIX 2)
    const uint32_t t = PIX == 1u ? tid >> 3 : tid >> 4, r = PIX == 1u ? tid & 7u : (tid >> 1) & 7u, hh = PIX == 1u ? 0u : tid & 1u;
    const uint32_t seg = blockIdx.x / p.spans, span = blockIdx.x - seg * p.spans;
    const uint32_t a0 = p.span_first[span], na = p.span_first[span + 1u] - a0;
    if (na == 0u) return;   // no active tile: the whole workgroup leaves
    const uint32_t ty = span / p.spans_x, txp = (span - ty * p.spans_x) * kTiles;
    const uint32_t nt = p.w - txp < kTiles ? p.w - txp : kTiles;
    const bool has_tile = t < nt;
    const uint32_t pos0 = ty * p.w + txp;              // the span's first tile (stream order)
    const uint32_t c = dec_chunk_of(p.geom, pos0), cb = dec_chunk_begin(p.geom, c);
    const uint32_t npre = pos0 - cb;                   // < 512 (roi_index_geometry)
    const uint32_t cstride = p.geom.cpf + 1u;
    const uint32_t f_begin = seg * p.fps;
    const uint64_t f_last = (uint64_t)f_begin + p.fps;
    const uint32_t f_end = f_last < p.n_frames ? (uint32_t)f_last : p.n_frames;
    const uint8_t *const end = p.stream + p.stream_bytes;
    const uint64_t L = p.n_labels;

    // ---- the map: this lane's labels and its place in the runs (the same for every frame) ----
    if (tid < kTiles) s_kind[tid] = 0u;
    __syncthreads();
    if (tid < na) s_kind[p.tile_pos[a0 + tid] - pos0] = p.tile_kind[a0 + tid];
    __syncthreads();
    const uint32_t kind = s_kind[t];
    const bool act = kind != 0u;
    uint32_t lab2[kNpx / 2];   // the lane's labels, two U16 per dword
    if (kind & kTraceMixed) {
        const uint16_t *b = p.blocks + 64ull * (kind & ~kTraceMixed) + 8u * r + 4u * hh;
        if constexpr (PIX == 1u) {
            const uint4 v = *reinterpret_cast<const uint4 *>(b);
            lab2[0] = v.x; lab2[1] = v.y; lab2[2] = v.z; lab2[3] = v.w;
        } else {
            const uint2 v = *reinterpret_cast<const uint2 *>(b);
            lab2[0] = v.x; lab2[1] = v.y;
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kNpx / 2; i++) lab2[i] = kind * 0x10001u;   // whole: the label; empty: 0
    }
    auto lab_of = [&](uint32_t i) __attribute__((always_inline)) -> uint32_t { return (lab2[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu; };
    // zm: label-0 pixels; bm: pixels that start a run other than the lane's first; le / lx: first / last label
    uint32_t zm = 0u, bm = 0u, le = 0u, lx = 0u;
#pragma unroll
    for (uint32_t i = 0; i < kNpx; i++) {
        const uint32_t l = lab_of(i);
        if (l == 0u) {
            zm |= 1u << i;
        } else {
            if (lx != 0u && l != lx) bm |= 1u << i;
            if (le == 0u) le = l;
            lx = l;
        }
    }
    // the last label in front of this lane (over the workgroup): max scan of (lane + 1) << 16 | label
    uint32_t lxprev;
    {
        const uint32_t key = lx != 0u ? ((tid + 1u) << 16) | lx : 0u;
        const uint32_t incl = wave_max_incl(key);
        if (lane == 63u) s_wmax[wave] = incl;
        __syncthreads();
        uint32_t before = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kTraceWaves; w++) before = w < wave && s_wmax[w] > before ? s_wmax[w] : before;
        uint32_t ex = (uint32_t)__shfl_up((int)incl, 1u, 64);
        if (lane == 0u) ex = 0u;
        ex = ex > before ? ex : before;
        lxprev = ex & 0xFFFFu;
    }
    if (lx == 0u) { le = lxprev; lx = lxprev; }        // no label of its own: the lane passes the run in front through
    const bool cont = le != 0u && le == lxprev;         // the lane's first run continues the run in front
    const bool uni = bm == 0u;                          // one run (or none)
    const bool join = uni && cont;                      // the lane's whole value belongs to the run in front
    const uint64_t bal_head = __ballot(!join), bal_cont = __ballot(cont);
    const uint64_t upto = lane == 63u ? ~0ull : (2ull << lane) - 1ull;
    const uint64_t hm = bal_head & upto;
    const uint32_t head = hm ? 63u - (uint32_t)__builtin_clzll(hm) : 0u;   // the lane where this lane's run starts in the wave
    const bool from_prev = hm == 0ull;                  // ... or the run came from the waves in front
    if (lane == 0u) { s_whole[wave] = bal_head == 0ull ? 1u : 0u; s_l0cont[wave] = (uint32_t)(bal_cont & 1ull); }
    __syncthreads();
    const bool nxt_cont = lane < 63u ? ((bal_cont >> (lane + 1u)) & 1ull) != 0ull
                                     : (wave + 1u < kTraceWaves && s_l0cont[wave + 1u] != 0u);
    // the scan's steps: bit k set when step k's source lane lies in this lane's run
    uint32_t take = 0u;
    {
        const uint32_t rl = lane & 15u;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (rl >= (1u << k) && lane - (1u << k) >= head) take |= 1u << k;
        if (((lane >> 4) & 1u) && (lane & ~15u) - 1u >= head) take |= 1u << 4;   // rows 1, 3 from lane 15 / 47
        if (lane >= 32u && 31u >= head) take |= 1u << 5;                         // rows 2, 3 from lane 31
    }

    // ---- the per-frame words of a group, one group ahead of their use: lane k < G holds frame g0 + k ----
    struct Words {
        uint32_t ok, base;
        uint64_t fo;
    };
    auto issue_words = [&](Words &wd, uint32_t g0) __attribute__((always_inline)) {
        const uint32_t g = g0 + (lane < G ? lane : 0u);
        wd.ok = 0u; wd.base = 0u; wd.fo = 0u;
        if (lane < G && g < f_end) {
            wd.ok = p.frame_ok[g];
            wd.fo = p.frame_offsets[g];
            wd.base = p.chunk_off[(size_t)g * cstride + c];
        }
    };

    // ---- one group of frames in flight ----
    struct Meta {
        uint32_t ok[G];            // uniform: frame accepted (and inside the segment)
        uint32_t g[G];             // uniform: the frame
        uint32_t base[G];          // uniform: payload words of the frame in front of the span's chunk
        const uint8_t *fb[G];      // uniform: the frame's bytes
        uint32_t d8[G], ml[G], mh[G];   // depth, minimum (PIX 2: its low / high byte) of this lane's tile (raw loads)
        uint32_t pre[G];           // this lane's dword of the depth bytes in front of the span (masked where used)
    };
    struct Pay {
        uint32_t a0[G], a1[G], a2[G];   // the aligned dwords around this lane's (half) row
        uint32_t dms[G];                // PIX 1: depth | minimum << 8 | byte shift << 16; PIX 2: depth | shift << 8 | minimum << 16
    };

    // As the projection's issue_meta: nothing consumes a loaded value here.  Only an active tile's minimum is read.
    auto issue_meta = [&](Meta &m, const Words &wd, uint32_t g0) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            m.ok[k] = 0u; m.base[k] = 0u; m.fb[k] = p.stream; m.d8[k] = 0u; m.ml[k] = 0u; m.pre[k] = 0u;
            m.g[k] = g0 + k;
            if constexpr (PIX == 2u) m.mh[k] = 0u;
            m.ok[k] = readlane(wd.ok, k);   // 0 past the segment
            if (m.ok[k]) {
                const uint64_t fo = (uint64_t)readlane((uint32_t)wd.fo, k) | ((uint64_t)readlane((uint32_t)(wd.fo >> 32), k) << 32);
                m.fb[k] = p.stream + fo;   // validated: the whole frame lies inside stream_bytes
                m.base[k] = readlane(wd.base, k);
                const uint8_t *darr = m.fb[k] + 24;
                const uint32_t tt = has_tile ? t : 0u;
                m.d8[k] = darr[pos0 + tt];
                if (act) {
                    if constexpr (PIX == 1u) {
                        m.ml[k] = darr[4u + p.T + pos0 + t];
                    } else {
                        m.ml[k] = darr[4u + p.T + 2u * (pos0 + t)];
                        m.mh[k] = darr[5u + p.T + 2u * (pos0 + t)];
                    }
                }
                const uint32_t head_b = (uint32_t)(reinterpret_cast<uintptr_t>(darr + cb) & 3u), ndw = (head_b + npre + 3u) >> 2;
                const uint8_t *a_lo = darr + cb - head_b;   // (pointer arithmetic: the load stays a global one)
                m.pre[k] = *reinterpret_cast<const uint32_t *>(a_lo + 4u * (tid < ndw ? tid : 0u));   // inside the frame
            }
        }
    };
    // the mask of the depth bytes [cb, pos0) in this lane's pre dword of frame fb
    auto pre_keep = [&](const uint8_t *fb) __attribute__((always_inline)) -> uint32_t {
        const uintptr_t a = reinterpret_cast<uintptr_t>(fb + 24 + cb);
        const uint32_t head_b = (uint32_t)(a & 3u), ndw = (head_b + npre + 3u) >> 2;
        if (tid >= ndw) return 0u;
        const uint32_t lo = 4u * tid < head_b ? head_b - 4u * tid : 0u;   // bytes in front of cb
        const uint32_t hi = head_b + npre - 4u * tid;                     // bytes before pos0
        return (hi >= 4u ? ~0u : (1u << (8u * hi)) - 1u) & ~((1u << (8u * lo)) - 1u);
    };

    // the group's tile offsets (one barrier) and its payload loads (active tiles only)
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
            const uint32_t pw = wave_sum(__builtin_amdgcn_sad_u8(m.pre[k] & pre_keep(m.fb[k]), 0u, 0u));
            if (lane == 63u) s_wsum[buf][k][0][wave] = incl[k];
            if (lane == 0u) s_wsum[buf][k][1][wave] = pw;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            uint32_t wbase = 0, PRE = 0;
#pragma unroll
            for (uint32_t w = 0; w < kTraceWaves; w++) {
                wbase += w < wave ? s_wsum[buf][k][0][w] : 0u;
                PRE += s_wsum[buf][k][1][w];
            }
            const uint32_t d = has_tile ? (m.d8[k] > kDmax ? kDmax : m.d8[k]) : 0u;
            const uint32_t woff = m.base[k] + PRE + wbase + incl[k] - d;   // payload words in front of the tile
            // PIX 2, the half row: byte r * d + h * (d / 2), a nibble further when d is odd; 4d bits (+ 4) <= 8 bytes
            const uint8_t *src = m.fb[k] + 32 + (PIX + 1ull) * p.T + 8ull * woff + r * d + hh * (d >> 1);
            const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
            const uint8_t *q8 = src - sh;   // (pointer arithmetic: the loads stay global ones)
            const bool need = m.ok[k] && act && d != 0u, tail = q8 + 12 > end;
            uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
            if (need && !tail) {
                const uint32_t *q32 = reinterpret_cast<const uint32_t *>(q8);
                w0 = q32[0]; w1 = q32[1]; w2 = q32[2];
            }
            if (need && tail) {   // the stream's last bytes: only those in front of stream_bytes
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

    // ---- the reduction of one group ----
    auto zero = []() __attribute__((always_inline)) -> R { R x; x.mm = 0u; x.s = 0u; x.q = 0u; return x; };
    auto fold = [](R &x, const R &y) __attribute__((always_inline)) {
        if constexpr (kMax || kMin) x.mm = pk_max_u16(x.mm, y.mm);
        if constexpr (kSum) x.s += y.s;
        if constexpr (kSq) x.q += y.q;
    };
    // one run of frame g -> the outputs (label lab, 1..L)
    auto flush = [&](const R &x, uint32_t lab, uint32_t g) __attribute__((always_inline)) {
        const uint64_t o = (uint64_t)g * L + (lab - 1u);
        if constexpr (kMax) atomicMax(p.ws_max + o, x.mm >> 16);
        if constexpr (kMin) atomicMin(p.ws_min + o, 0xFFFFu - (x.mm & 0xFFFFu));
        if constexpr (kSum) atomicAdd(reinterpret_cast<unsigned long long *>(p.out_sum + o), (unsigned long long)x.s);
        if constexpr (kSq) atomicAdd(reinterpret_cast<unsigned long long *>(p.out_sumsq + o), (unsigned long long)x.q);
    };
    uint32_t tb = 0;
    auto reduce = [&](const Meta &m, const Pay &q) __attribute__((always_inline)) {
        uint32_t any = 0;
#pragma unroll
        for (uint32_t k = 0; k < G; k++) any |= m.ok[k];
        if (!any) return;
        R E[G], S[G];
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            E[k] = zero(); S[k] = zero();
            if (!m.ok[k]) continue;   // rejected (or past the segment): its row is not touched
            // this lane's pixels
            uint32_t v[kNpx];
            if constexpr (PIX == 1u) {
                const uint32_t d = q.dms[k] & 0xFFu, sh = q.dms[k] >> 16;
                const uint32_t mm = ((q.dms[k] >> 8) & 0xFFu) * 0x01010101u;
                const uint64_t bits = (uint64_t)__builtin_amdgcn_alignbyte(q.a1[k], q.a0[k], sh) |
                                      ((uint64_t)__builtin_amdgcn_alignbyte(q.a2[k], q.a1[k], sh) << 32);
                uint32_t px[2];
                expand_row(bits, d, px[0], px[1]);
                px[0] = add_bytes(px[0], mm);
                px[1] = add_bytes(px[1], mm);
#pragma unroll
                for (uint32_t i = 0; i < 8u; i++) v[i] = (px[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
            } else {
                const uint32_t d = q.dms[k] & 0xFFu, sh = (q.dms[k] >> 8) & 0xFFu, so = 4u * hh * (d & 1u);
                const uint32_t m32 = d >= 16u ? 0xFFFFu : (1u << d) - 1u, mn2 = (q.dms[k] >> 16) * 0x00010001u;
                const bool c2 = 2u * d >= 32u, c3 = 3u * d >= 32u;
                const uint32_t x0 = __builtin_amdgcn_alignbyte(q.a1[k], q.a0[k], sh);
                const uint32_t x1 = __builtin_amdgcn_alignbyte(q.a2[k], q.a1[k], sh);
                uint32_t e[2];
                cut_four16(__builtin_amdgcn_alignbit(x1, x0, so), x1 >> so, d, m32, mn2, c2, c3, e[0], e[1]);
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) v[i] = (e[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu;
            }
            // the lane's runs: E the first, X (in S) the last, those between flushed here
            R cur = zero();
            if (zm == 0u && bm == 0u) {   // a whole tile's row: one run
#pragma unroll
                for (uint32_t i = 0; i < kNpx; i++) {
                    R x; x.mm = (v[i] << 16) | (0xFFFFu - v[i]); x.s = v[i]; x.q = (TraceSq<PIX>)(v[i] * v[i]);
                    fold(cur, x);
                }
            } else if (act) {
                uint32_t curlab = 0u;
#pragma unroll
                for (uint32_t i = 0; i < kNpx; i++) {
                    if ((bm >> i) & 1u) {
                        if ((bm & (0u - bm)) == (1u << i)) E[k] = cur;   // the lane's first run ends here
                        else flush(cur, curlab, m.g[k]);                // a run between the first and the last
                        cur = zero();
                    }
                    if (!((zm >> i) & 1u)) {
                        R x; x.mm = (v[i] << 16) | (0xFFFFu - v[i]); x.s = v[i]; x.q = (TraceSq<PIX>)(v[i] * v[i]);
                        fold(cur, x);
                        curlab = lab_of(i);
                    }
                }
            }
            // the segmented scan over the wave: S = this run's value from its head lane to here
            S[k] = cur;
            scan_step<STATS, PIX, 0x111, 0xF>(S[k], (take & 1u) != 0u);
            scan_step<STATS, PIX, 0x112, 0xF>(S[k], (take & 2u) != 0u);
            scan_step<STATS, PIX, 0x114, 0xF>(S[k], (take & 4u) != 0u);
            scan_step<STATS, PIX, 0x118, 0xF>(S[k], (take & 8u) != 0u);
            scan_step<STATS, PIX, 0x142, 0xA>(S[k], (take & 16u) != 0u);
            scan_step<STATS, PIX, 0x143, 0xC>(S[k], (take & 32u) != 0u);
            if (lane == 63u) {
                s_tail[tb][k][wave][0] = S[k].mm;
                s_tail[tb][k][wave][1] = S[k].s;
                s_tail[tb][k][wave][2] = (uint32_t)S[k].q;
                s_tail[tb][k][wave][3] = PIX == 1u ? 0u : (uint32_t)((uint64_t)S[k].q >> 32);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!m.ok[k]) continue;
            // the run that reaches this wave from the waves in front
            R carry = zero();
#pragma unroll
            for (uint32_t w = 0; w + 1u < kTraceWaves; w++) {
                if (w < wave) {
                    R x;
                    x.mm = s_tail[tb][k][w][0];
                    x.s = s_tail[tb][k][w][1];
                    if constexpr (PIX == 1u) x.q = s_tail[tb][k][w][2];
                    else x.q = (uint64_t)s_tail[tb][k][w][2] | ((uint64_t)s_tail[tb][k][w][3] << 32);
                    if (!s_whole[w]) carry = zero();
                    fold(carry, x);
                }
            }
            if (from_prev) fold(S[k], carry);
            R prev;   // the run in front of this lane, up to the lane in front
            prev.mm = (uint32_t)__shfl_up((int)S[k].mm, 1u, 64);
            prev.s = (uint32_t)__shfl_up((int)S[k].s, 1u, 64);
            if constexpr (PIX == 1u) {
                prev.q = (uint32_t)__shfl_up((int)S[k].q, 1u, 64);
            } else {
                prev.q = (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)S[k].q, 1u, 64) |
                         ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(S[k].q >> 32), 1u, 64) << 32);
            }
            if (lane == 0u) prev = carry;
            if (!uni && le != 0u) {   // the lane's first run ends in this lane
                R x = E[k];
                if (cont) fold(x, prev);
                flush(x, le, m.g[k]);
            }
            if (lx != 0u && !nxt_cont) flush(S[k], lx, m.g[k]);   // the run ends with this lane
        }
        tb ^= 1u;
    };

    // ---- the pipeline: reduce group k while group k + 1's payload and group k + 2's depth bytes load ----
    Meta m_cur, m_nxt, m_nn;
    Pay q_cur, q_nxt;
    Words w_nn;
    issue_words(w_nn, f_begin);
    issue_meta(m_cur, w_nn, f_begin);
    issue_payload(m_cur, q_cur);
    issue_words(w_nn, f_begin + G);
    issue_meta(m_nxt, w_nn, f_begin + G);
    issue_words(w_nn, f_begin + 2u * G);
    for (uint32_t g0 = f_begin; g0 < f_end; g0 += G) {
        issue_payload(m_nxt, q_nxt);
        issue_meta(m_nn, w_nn, g0 + 2u * G);
        issue_words(w_nn, g0 + 3u * G);
        reduce(m_cur, q_cur);
        m_cur = m_nxt;
        q_cur = q_nxt;
        m_nxt = m_nn;
    }
}

// The accepted frames' rows before the trace kernel: sums 0, the max / min workspace at the empty values (0, pix_max).
// One thread per (frame, label).
__global__ __launch_bounds__(kTraceRowThreads) void trace_init_kernel(TraceParams p) {
    const uint64_t n = (uint64_t)p.n_frames * p.n_labels;
    const uint64_t i = (uint64_t)blockIdx.x * kTraceRowThreads + threadIdx.x;
    if (i >= n) return;
    if (!p.frame_ok[i / p.n_labels]) return;   // a rejected frame's row is left as it is
    if (p.out_sum) p.out_sum[i] = 0ull;
    if (p.out_sumsq) p.out_sumsq[i] = 0ull;
    if (p.ws_max) p.ws_max[i] = 0u;
    if (p.ws_min) p.ws_min[i] = p.pix_max;
}

// The accepted frames' max / min rows from the workspace.  One thread per (frame, label).
template <uint32_t PIX>
__global__ __launch_bounds__(kTraceRowThreads) void trace_finish_kernel(TraceParams p) {
    typedef TracePix<PIX> Pix;
    const uint64_t n = (uint64_t)p.n_frames * p.n_labels;
    const uint64_t i = (uint64_t)blockIdx.x * kTraceRowThreads + threadIdx.x;
    if (i >= n) return;
    if (!p.frame_ok[i / p.n_labels]) return;
    if (p.out_max) reinterpret_cast<Pix *>(p.out_max)[i] = (Pix)p.ws_max[i];
    if (p.out_min) reinterpret_cast<Pix *>(p.out_min)[i] = (Pix)p.ws_min[i];
}

typedef void (*TraceKernel)(TraceParams);
struct TraceTable {
    TraceKernel k[16];   // [stats]: trace_kernel<stats, PIX>, 1..15
};

template <uint32_t PIX, uint32_t... S>
static constexpr TraceTable trace_table(std::integer_sequence<uint32_t, S...>) {
    return {{nullptr, trace_kernel<S + 1u, PIX>...}};
}

hipError_t launch_traces(const TraceParams &p, uint32_t stats, uint32_t pix, hipStream_t s) {
    static const TraceTable tables[2] = {trace_table<1>(std::make_integer_sequence<uint32_t, 15>()),
                                         trace_table<2>(std::make_integer_sequence<uint32_t, 15>())};
    if (stats < 1u || stats > kProjAll || (pix != 1u && pix != 2u)) return hipErrorInvalidValue;
    const uint64_t rows = (uint64_t)p.n_frames * p.n_labels;
    const uint32_t rgrid = (uint32_t)((rows + kTraceRowThreads - 1u) / kTraceRowThreads);   // (the host keeps it below 2^31)
    hipLaunchKernelGGL(trace_init_kernel, dim3(rgrid), dim3(kTraceRowThreads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint64_t grid = (uint64_t)p.spans * p.segments;
    if (grid) {
        hipLaunchKernelGGL(tables[pix - 1u].k[stats], dim3((uint32_t)grid), dim3(kTraceThreads), 0, s, p);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (!(stats & (kProjMax | kProjMin))) return hipSuccess;
    const TraceKernel finish = pix == 1u ? trace_finish_kernel<1> : trace_finish_kernel<2>;
    hipLaunchKernelGGL(finish, dim3(rgrid), dim3(kTraceRowThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
