// dbde_lag_kernels.hip -- lag projections for MI355X (gfx950, wave64): per pixel of the rw x rh window, over the pairs
// (a, b) = (p_{f - lag}, p_f) of frames `lag` apart, product = sum a * b, pairsum = sum (a + b), absdiff = sum |b - a|,
// sqdiff = sum (b - a)^2 and maxdiff = max |b - a|, straight from the compressed bytes (no image is written).
// DESIGN.md 4.21.
//
// lag_kernel<STATS, PIX>: STATS = the instance's statistics (kLagInstanceOf: 3, 28 or 31), PIX = 1 for DBDE frames,
// PIX = 2 for DBDE16 frames.  The launch shape and the load pipeline are project_kernel's (dbde_proj_pipeline.h), as
// counts_kernel took them: one 256-lane workgroup per (frame segment, window tile row, piece of kProjTilesOf(PIX)
// tiles), one lane per tile row (PIX 2: per half row), the frames walked in groups of kLagGroup with the payload loads
// of group k + 1, the depth / minimum loads of group k + 2 and the per-frame words of group k + 3 in flight while group
// k is folded, one barrier per group.  The body is this file's own.
//
// The history.  A lane owns the same 8 bytes of decoded pixels (8 U8 or 4 U16) of every frame, so the partner of frame
// f is what the lane itself decoded lag frames earlier.  It lives in a per-lane ring in LDS, hist[kLagMax][256] of 8
// bytes, slot = frame index mod 8: an accepted frame reads slot (f - lag) mod 8, then writes slot f mod 8 (the same slot
// for lag 8: the read comes first).  A lane reads only what it wrote, so the ring needs no barrier.  Consecutive lanes
// hold consecutive 8-byte elements: a 64-bit LDS read serves 32 lanes = 64 consecutive dwords = 64 banks per cycle, a
// 64-bit write 16 lanes = 32 dwords = 32 banks: no conflicts.  Whether each of the last 8 frames was accepted is a
// uniform shift register, valid = valid << 1 | ok; a rejected frame writes nothing and its stale slot is never read.
//
// The segments.  Segment s counts the pairs whose later frame lies in [s * fps, (s + 1) * fps) and in
// [max(lead, lag), n_frames).  It starts lag frames in front of the first of them and folds those as history only:
// decoded, stored to the ring, nothing accumulated.  `lead` is the same mechanism applied to the call.
//
// The value.  All sums are exact integers: per lane U32 for DBDE (65,536 * 255^2 < 2^32, 65,536 * 510 < 2^32), for
// DBDE16 U64 for product, sqdiff and pairsum (65,536 * 131,070 = 2^33) and U32 for absdiff (65,536 * 65,535 < 2^32),
// over the at most kProjMaxFramesPerSegment counted frames of a segment.  With one segment each lane writes its window
// pixels of the requested planes (combined with the old value when accumulating); with more, the per-segment partials
// go to the workspace and lag_combine_kernel (one thread per window pixel) adds them in U64 (max for maxdiff).
#include "dbde_lag_kernels.h"

#include <type_traits>

#include "dbde_proj_pipeline.h"

namespace dbde {

namespace {

// The two scalars: *p.out_count = accepted frames of [lead, n_frames), *p.out_pairs = frames f of
// [max(lead, lag), n_frames) with f and f - lag both accepted (added to what they hold when accumulating).  Whole
// workgroup.
__device__ void write_scalars(const LagParams &p) {
    __shared__ uint32_t s_c[2][kProjWaves];
    const uint32_t tid = threadIdx.x;
    const uint32_t first = p.lead > p.lag ? p.lead : p.lag;
    uint32_t c = 0, pr = 0;
    for (uint32_t g = tid; g < p.n_frames; g += kProjThreads) {
        const bool ok = p.frame_ok[g] != 0u;
        c += ok && g >= p.lead ? 1u : 0u;
        if (ok && g >= first) pr += p.frame_ok[g - p.lag] != 0u ? 1u : 0u;
    }
    c = wave_sum(c);
    pr = wave_sum(pr);
    if ((tid & 63u) == 0u) { s_c[0][tid >> 6] = c; s_c[1][tid >> 6] = pr; }
    __syncthreads();
    if (tid == 0) {
        uint64_t tc = 0, tp = 0;
        for (uint32_t k = 0; k < kProjWaves; k++) { tc += s_c[0][k]; tp += s_c[1][k]; }
        *p.out_count = (p.accumulate ? *p.out_count : 0ull) + tc;
        *p.out_pairs = (p.accumulate ? *p.out_pairs : 0ull) + tp;
    }
}

}  // namespace

template <uint32_t STATS, uint32_t PIX>
__global__ __launch_bounds__(kProjThreads) void lag_kernel(LagParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    static_assert(STATS >= 1u && STATS <= kLagAll, "a set of the five statistics");
    constexpr uint32_t G = kLagGroup, kNpx = 8u / PIX;                                   // kNpx: pixels per lane
    constexpr uint32_t kPerDw = 4u / PIX, kBits = 8u * PIX, kMask = (1u << kBits) - 1u;   // pixels per dword
    constexpr bool kProd = (STATS & kLagProduct) != 0u, kPsum = (STATS & kLagPairSum) != 0u, kAbs = (STATS & kLagAbsDiff) != 0u,
                   kSq = (STATS & kLagSqDiff) != 0u, kMaxd = (STATS & kLagMaxDiff) != 0u;
    typedef typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type Px;
    typedef typename std::conditional<PIX == 1u, uint32_t, uint64_t>::type Wide;   // product, pairsum, sqdiff of a segment
    typedef ProjPipeline<PIX, G, LagParams> Pipe;
    __shared__ uint32_t s_wsum[2][G][2][kProjWaves];
    __shared__ uint2 s_hist[kLagMax][kProjThreads];   // the ring: this lane's decoded (half) row of the last 8 frames

    const ProjPiece<PIX> pc = proj_piece<PIX>(p);
    const uint32_t tid = pc.tid, t = pc.t, r = pc.r, hh = pc.hh, seg = pc.seg, ty = pc.ty, txp = pc.txp;
    // the counted frames [c_lo, c_hi) of this segment and the lag history frames in front of them
    const uint32_t lag = p.lag, first = p.lead > lag ? p.lead : lag;
    const uint64_t s_lo = (uint64_t)seg * p.fps, s_hi = s_lo + p.fps;
    const uint32_t c_hi = s_hi < p.n_frames ? (uint32_t)s_hi : p.n_frames;
    const uint32_t c_lo = s_lo > first ? (uint32_t)s_lo : first;   // (>= lag)
    const bool any_pair = c_lo < c_hi;
    const uint32_t f_begin = any_pair ? c_lo - lag : 0u, f_end = any_pair ? c_hi : 0u;

    // ---- this lane's pixels in the window and the accumulators ----
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const int yy = 8 * (int)ty + (int)r;
    const int xx0 = 8 * (int)(txp + t) + 4 * (int)hh;                  // the lane's first pixel column
    const bool row_in = pc.has_tile && yy >= p.y0 && yy < p.y0 + p.rh;
    const uint64_t row0 = row_in ? (uint64_t)(yy - p.y0) * (uint64_t)p.rw : 0u;

    Wide a_prod[kNpx], a_psum[kNpx], a_sq[kNpx];
    uint32_t a_abs[kNpx], a_max[kNpx];
#pragma unroll
    for (uint32_t i = 0; i < kNpx; i++) {
        a_prod[i] = 0u; a_psum[i] = 0u; a_sq[i] = 0u; a_abs[i] = 0u; a_max[i] = 0u;
    }

    // the kPerDw pixels of dword h: a = the earlier frame's, b = this frame's
    auto tally = [&](uint32_t h, uint32_t va, uint32_t vb) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t i = 0; i < kPerDw; i++) {
            const uint32_t j = kPerDw * h + i;
            const uint32_t a = (va >> (kBits * i)) & kMask, b = (vb >> (kBits * i)) & kMask;
            if constexpr (kProd) a_prod[j] += (Wide)a * (Wide)b;
            if constexpr (kPsum) a_psum[j] += (Wide)(a + b);
            if constexpr (kAbs || kSq || kMaxd) {
                const uint32_t df = __builtin_amdgcn_sad_u16(a, b, 0u);   // |b - a| (the high halves are 0)
                if constexpr (kAbs) a_abs[j] += df;
                if constexpr (kSq) a_sq[j] += (Wide)df * (Wide)df;
                if constexpr (kMaxd) a_max[j] = a_max[j] > df ? a_max[j] : df;
            }
        }
    };
    uint32_t valid = 0u;   // uniform: bit j = frame (this one - 1 - j) was accepted and stored to the ring
    auto accumulate = [&](const typename Pipe::Meta &m, const typename Pipe::Pay &q, uint32_t g0) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            const uint32_t f = g0 + k;
            if (m.ok[k]) {   // a rejected frame (or one past the segment) is no partner and stores nothing
                uint32_t e[2];
                cut_row<PIX>(q.a0[k], q.a1[k], q.a2[k], q.dms[k], hh, e[0], e[1]);
                if (f >= c_lo && ((valid >> (lag - 1u)) & 1u)) {   // uniform: the pair (f - lag, f) is counted
                    const uint2 old = s_hist[(f - lag) & (kLagMax - 1u)][tid];
                    tally(0u, old.x, e[0]);
                    tally(1u, old.y, e[1]);
                }
                s_hist[f & (kLagMax - 1u)][tid] = make_uint2(e[0], e[1]);   // after the read: the same slot for lag 8
            }
            valid = (valid << 1) | (m.ok[k] ? 1u : 0u);
        }
    };

    // ---- the pipeline: fold group k while group k + 1's payload and group k + 2's depth bytes load ----
    uint32_t buf = 0;
    Pipe pl{p, pc, s_wsum, p.stream + p.stream_bytes, buf};
    typename Pipe::Meta m_cur, m_nxt, m_nn;
    typename Pipe::Pay q_cur, q_nxt;
    typename Pipe::Words w_nn;
    pl.issue_words(w_nn, f_begin, f_end);
    pl.issue_meta(m_cur, w_nn);
    pl.issue_payload(m_cur, q_cur);
    pl.issue_words(w_nn, f_begin + G, f_end);
    pl.issue_meta(m_nxt, w_nn);
    pl.issue_words(w_nn, f_begin + 2u * G, f_end);
    for (uint32_t g0 = f_begin; g0 < f_end; g0 += G) {
        pl.issue_payload(m_nxt, q_nxt);
        pl.issue_meta(m_nn, w_nn);
        pl.issue_words(w_nn, g0 + 3u * G, f_end);
        accumulate(m_cur, q_cur, g0);
        m_cur = m_nxt;
        q_cur = q_nxt;
        m_nxt = m_nn;
    }

    // ---- the window's pixels of this lane -> the requested planes, or this segment's partials ----
    if (row_in) {
        const bool direct = p.segments == 1u, acc = direct && p.accumulate;
        const uint64_t so = (uint64_t)seg * P;
#pragma unroll
        for (uint32_t i = 0; i < kNpx; i++) {
            const int xx = xx0 + (int)i;
            if (xx < p.x0 || xx >= p.x0 + p.rw) continue;
            const uint64_t o = row0 + (uint64_t)(xx - p.x0);
            if (direct) {
                if constexpr (kProd) if (p.out_product) p.out_product[o] = (acc ? p.out_product[o] : 0ull) + a_prod[i];
                if constexpr (kPsum) if (p.out_pairsum) p.out_pairsum[o] = (acc ? p.out_pairsum[o] : 0ull) + a_psum[i];
                if constexpr (kAbs) if (p.out_absdiff) p.out_absdiff[o] = (acc ? p.out_absdiff[o] : 0ull) + a_abs[i];
                if constexpr (kSq) if (p.out_sqdiff) p.out_sqdiff[o] = (acc ? p.out_sqdiff[o] : 0ull) + a_sq[i];
                if constexpr (kMaxd) if (p.out_maxdiff) {
                    Px *const q = static_cast<Px *>(p.out_maxdiff) + o;
                    const uint32_t old = acc ? (uint32_t)*q : 0u;
                    *q = (Px)(old > a_max[i] ? old : a_max[i]);
                }
            } else {
                if constexpr (kProd) if (p.ws_product) static_cast<Wide *>(p.ws_product)[so + o] = a_prod[i];
                if constexpr (kPsum) if (p.ws_pairsum) static_cast<Wide *>(p.ws_pairsum)[so + o] = a_psum[i];
                if constexpr (kAbs) if (p.ws_absdiff) p.ws_absdiff[so + o] = a_abs[i];
                if constexpr (kSq) if (p.ws_sqdiff) static_cast<Wide *>(p.ws_sqdiff)[so + o] = a_sq[i];
                if constexpr (kMaxd) if (p.ws_maxdiff) static_cast<Px *>(p.ws_maxdiff)[so + o] = (Px)a_max[i];
            }
        }
    }
    if (p.segments == 1u && blockIdx.x == 0u) write_scalars(p);
}

// Segments > 1: prior (ACC: what the planes hold) + partial 0 + partial 1 + ... in U64, the maximum for maxdiff.  One
// thread per window pixel; the partials are [segments][rw * rh], so each read is coalesced.
template <uint32_t PIX, bool ACC>
__global__ __launch_bounds__(kProjCombineThreads) void lag_combine_kernel(LagParams p) {
    typedef typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type Px;
    typedef typename std::conditional<PIX == 1u, uint32_t, uint64_t>::type Wide;
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const uint64_t i = (uint64_t)blockIdx.x * kProjCombineThreads + threadIdx.x;
    if (i < P) {
        if (p.out_product) {
            uint64_t v = ACC ? p.out_product[i] : 0ull;
            for (uint32_t s = 0; s < p.segments; s++) v += static_cast<const Wide *>(p.ws_product)[(uint64_t)s * P + i];
            p.out_product[i] = v;
        }
        if (p.out_pairsum) {
            uint64_t v = ACC ? p.out_pairsum[i] : 0ull;
            for (uint32_t s = 0; s < p.segments; s++) v += static_cast<const Wide *>(p.ws_pairsum)[(uint64_t)s * P + i];
            p.out_pairsum[i] = v;
        }
        if (p.out_absdiff) {
            uint64_t v = ACC ? p.out_absdiff[i] : 0ull;
            for (uint32_t s = 0; s < p.segments; s++) v += p.ws_absdiff[(uint64_t)s * P + i];
            p.out_absdiff[i] = v;
        }
        if (p.out_sqdiff) {
            uint64_t v = ACC ? p.out_sqdiff[i] : 0ull;
            for (uint32_t s = 0; s < p.segments; s++) v += static_cast<const Wide *>(p.ws_sqdiff)[(uint64_t)s * P + i];
            p.out_sqdiff[i] = v;
        }
        if (p.out_maxdiff) {
            Px *const q = static_cast<Px *>(p.out_maxdiff) + i;
            uint32_t v = ACC ? (uint32_t)*q : 0u;
            for (uint32_t s = 0; s < p.segments; s++) {
                const uint32_t x = static_cast<const Px *>(p.ws_maxdiff)[(uint64_t)s * P + i];
                v = v > x ? v : x;
            }
            *q = (Px)v;
        }
    }
    if (blockIdx.x == 0u) write_scalars(p);
}

uint64_t lag_partial_bytes(uint32_t bit, uint32_t segments, uint64_t pixels, uint32_t pix) {
    if (segments <= 1u) return 0;
    const uint64_t n = (uint64_t)segments * pixels;
    const uint64_t width = bit == kLagMaxDiff ? pix : bit == kLagAbsDiff ? 4u : 4u * pix;
    return (width * n + 15u) & ~(uint64_t)15;
}

uint64_t lag_workspace_bytes(uint32_t stats, uint32_t segments, uint64_t pixels, uint32_t pix) {
    uint64_t total = 0;
    for (uint32_t bit = 1u; bit <= kLagMaxDiff; bit <<= 1)
        if (stats & bit) total += lag_partial_bytes(bit, segments, pixels, pix);
    return total;
}

typedef void (*LagKernel)(LagParams);

hipError_t launch_lag(const LagParams &p, uint32_t stats, uint32_t pix, hipStream_t s) {
    if (stats < 1u || stats > kLagAll || (pix != 1u && pix != 2u) || p.lag < 1u || p.lag > kLagMax || p.lead > p.n_frames)
        return hipErrorInvalidValue;
    const uint32_t inst = kLagInstanceOf(stats);
    const LagKernel kernel = pix == 1u ? (inst == 3u ? lag_kernel<3, 1> : inst == 28u ? lag_kernel<28, 1> : lag_kernel<31, 1>)
                                       : (inst == 3u ? lag_kernel<3, 2> : inst == 28u ? lag_kernel<28, 2> : lag_kernel<31, 2>);
    const uint32_t grid = p.pieces * p.rows * p.segments;   // (the host keeps it below 2^31)
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kProjThreads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.segments == 1u) return e;
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const uint32_t cgrid = (uint32_t)((P + kProjCombineThreads - 1u) / kProjCombineThreads);
    const LagKernel combine = pix == 1u ? (p.accumulate ? lag_combine_kernel<1, true> : lag_combine_kernel<1, false>)
                                        : (p.accumulate ? lag_combine_kernel<2, true> : lag_combine_kernel<2, false>);
    hipLaunchKernelGGL(combine, dim3(cgrid), dim3(kProjCombineThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
