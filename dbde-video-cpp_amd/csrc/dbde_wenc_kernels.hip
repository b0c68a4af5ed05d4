// dbde_wenc_kernels.hip -- window encode on MI355X (gfx950): the rw x rh window at (x, y) of each pitched source image
// as a DBDE (PIX = 1) or DBDE16 (PIX = 2) frame, byte for byte what the frame encoders write for a contiguous copy of the
// window.  The window is never copied: its rows are fetched where they lie.
//
// One template, encode_window_kernel<PIX>, built like enc16_kernel (dbde16_kernels.hip): persistent workgroups, a chunk =
// 256 lanes of tiles in stream order, chunk ids = arrival ranks (static once all workgroups have been seen, tickets
// otherwise), a chunk's word count published as an 8-byte record, prefixes = two-level sums of records, the payload
// packed into an LDS image while the record travels.  New here is the fetch:
//   * tiles are counted from the WINDOW's corner; a lane holds one UNIT -- PIX = 1: two adjacent tiles (pairs never leave
//     a tile row: ceil(w / 2) lanes per row), PIX = 2: one tile -- 16 source bytes per image row either way, one
//     nontemporal 16-byte load at whatever byte address they have;
//   * the image row is clamped to rh - 1 (the rows below a window are real source rows), and the bytes of columns at
//     or beyond rw (real pixels, or pitch padding) are replaced IN REGISTERS by the row's last valid pixel;
//   * a lane whose 16-byte loads would pass images + image_bytes (the last rows of the last frame only), and every
//     lane of a window narrower than 16 bytes, fetches its valid bytes one by one instead.
#include "dbde_wenc_kernels.h"

#include "dbde_bits.h"
#include "dbde_device.h"
#include "dbde_kernels.h"

namespace dbde {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef u32x4_t __attribute__((aligned(1))) u32x4_unaligned;
typedef unsigned long long u64a;
constexpr u64a kReady = 1ull << 63;

__device__ __forceinline__ void store_u32_bytes(uint8_t *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
__device__ __forceinline__ void store_u64_any(uint8_t *p, uint64_t v) { __builtin_memcpy(p, &v, 8); }

__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}
// Wave-wide: sums of four record ranges (at most 64 records each: lane l reads record l of every range in one poll),
// waiting until every record is published.  0 after 2 s (the caller raises the sticky failure word).  enc16_kernel's.
__device__ __forceinline__ uint32_t sum_records(const u64a *r0, uint32_t n0, const u64a *r1, uint32_t n1, const u64a *r2, uint32_t n2,
                                                const u64a *r3, uint32_t n3, uint32_t lane, uint64_t t_start,
                                                uint64_t &s0, uint64_t &s1, uint64_t &s2, uint64_t &s3) {
    u64a w0 = kReady, w1 = kReady, w2 = kReady, w3 = kReady;
    for (;;) {
        if (lane < n0 && w0 == kReady) w0 = __hip_atomic_load(&r0[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane < n1 && w1 == kReady) w1 = __hip_atomic_load(&r1[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane < n2 && w2 == kReady) w2 = __hip_atomic_load(&r2[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane < n3 && w3 == kReady) w3 = __hip_atomic_load(&r3[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__all((int)(((w0 & w1 & w2 & w3) >> 63) & 1ull))) break;
        if (wall_clock64() - t_start > 200000000ull) return 0u;   // 2 s at 100 MHz: give up, loudly
        __builtin_amdgcn_s_sleep(1);
        // records not there yet read as 0: mark them "to be read again"
        w0 = (w0 & kReady) ? w0 : kReady; w1 = (w1 & kReady) ? w1 : kReady; w2 = (w2 & kReady) ? w2 : kReady; w3 = (w3 & kReady) ? w3 : kReady;
    }
    s0 = wave_sum64(lane < n0 ? (w0 & ~kReady) : 0ull); s1 = wave_sum64(lane < n1 ? (w1 & ~kReady) : 0ull);
    s2 = wave_sum64(lane < n2 ? (w2 & ~kReady) : 0ull); s3 = wave_sum64(lane < n3 ? (w3 & ~kReady) : 0ull);
    return 1u;
}

// min and max over the 64 U16 pixels held in 32 dwords (DBDE16 tile)
__device__ __forceinline__ void tile_minmax_u16(const uint32_t (&v)[32], uint32_t &mn, uint32_t &mx) {
    uint32_t lo = v[0], hi = v[0];
#pragma unroll
    for (int i = 1; i < 32; i++) { lo = pk_min_u16(lo, v[i]); hi = pk_max_u16(hi, v[i]); }
    mn = (lo & 0xFFFFu) < (lo >> 16) ? (lo & 0xFFFFu) : (lo >> 16);
    mx = (hi & 0xFFFFu) > (hi >> 16) ? (hi & 0xFFFFu) : (hi >> 16);
}

// A tile's payload words into the LDS image, straight-line funnel over its rows (every row stores the word it is
// filling; the tile's 64 * d bits end on a word boundary).  A tile without payload writes the trash word.
// DBDE: 8 rows of 8 * d <= 64 bits.
__device__ __forceinline__ void pack_tile8(const uint32_t (&v)[16], uint32_t mn, uint32_t d, uint64_t *s_pay, uint32_t q0) {
    const uint32_t mn4 = mn * 0x01010101u;   // every byte >= mn: no borrow crosses a byte
    const uint32_t nb = 8u * d;
    uint32_t q = d ? q0 : kWencPayWords;
    uint64_t acc = 0;
    uint32_t fill = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint64_t bits = pack_row(v[2 * r] - mn4, v[2 * r + 1] - mn4, d);
        const uint64_t merged = acc | (bits << fill);
        s_pay[q < kWencPayWords ? q : kWencPayWords] = merged;
        const uint32_t nf = fill + nb;
        const bool emit = nf >= 64u;
        acc = emit ? ((bits >> 1) >> (63u - fill)) : merged;
        fill = nf & 63u;
        q += emit ? 1u : 0u;
    }
}
// DBDE16: 16 half rows of 4 * d <= 64 bits (pack_tile16 of dbde16_kernels.hip).
__device__ __forceinline__ void pack_tile16w(const uint32_t (&v)[32], uint32_t mn, uint32_t d, uint64_t *s_pay, uint32_t q0) {
    const uint32_t mn2 = mn * 0x00010001u;   // every 16-bit half >= mn: no borrow crosses a half
    const uint32_t nb = 4u * d;
    uint32_t q = d ? q0 : kWencPayWords;
    uint64_t acc = 0;
    uint32_t fill = 0;
#pragma unroll
    for (int h = 0; h < 16; h++) {
        const uint64_t bits = pack_four16(v[2 * h] - mn2, v[2 * h + 1] - mn2, d);
        const uint64_t merged = acc | (bits << fill);
        s_pay[q < kWencPayWords ? q : kWencPayWords] = merged;
        const uint32_t nf = fill + nb;
        const bool emit = nf >= 64u;
        acc = emit ? ((bits >> 1) >> (63u - fill)) : merged;
        fill = nf & 63u;
        q += emit ? 1u : 0u;
    }
}

// `n` words of the LDS image to dst (the chunk's payload is contiguous): 16-byte stores where dst is word-aligned.
__device__ __forceinline__ void copy_out(const uint64_t *s_pay, uint8_t *dst, uint32_t n, uint32_t tid) {
    if ((reinterpret_cast<uintptr_t>(dst) & 7u) == 0u) {   // 16-byte stores between a possible odd first and last word
        const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(dst) >> 3) & 1u;
        const uint32_t h1 = head < n ? head : n;
        if (tid == 0 && h1) *reinterpret_cast<uint64_t *>(dst) = s_pay[0];
        const uint32_t pairs = (n - h1) >> 1;
        typedef uint64_t u64x2_t __attribute__((ext_vector_type(2)));
        for (uint32_t i = tid; i < pairs; i += kWencThreads) {
            u64x2_t q = {s_pay[h1 + 2u * i], s_pay[h1 + 2u * i + 1u]};
            *reinterpret_cast<u64x2_t *>(dst + 8ull * (h1 + 2u * i)) = q;
        }
        if (tid == 64u && ((n - h1) & 1u)) *reinterpret_cast<uint64_t *>(dst + 8ull * (n - 1u)) = s_pay[n - 1u];
    } else {
        for (uint32_t i = tid; i < n; i += kWencThreads) store_u64_any(dst + 8ull * i, s_pay[i]);
    }
}

// The 16 bytes of one unit row whose first `nvb` bytes (a whole number of pixels, >= one) are inside the window: the
// others become copies of the last valid pixel.
template <int PIX>
__device__ __forceinline__ void extend_row(uint32_t (&q)[4], uint32_t nvb) {
    const uint32_t lb = nvb - (uint32_t)PIX;                  // byte offset of the last valid pixel
    const uint32_t ld = lb < 4u ? q[0] : (lb < 8u ? q[1] : (lb < 12u ? q[2] : q[3]));
    const uint32_t L = ld >> (8u * (lb & 3u));
    const uint32_t fillv = PIX == 1 ? (L & 0xFFu) * 0x01010101u : (L & 0xFFFFu) * 0x00010001u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t b0 = 4u * (uint32_t)j;
        if (b0 >= nvb) q[j] = fillv;
        else if (b0 + 4u > nvb) {
            const uint32_t keep = (1u << (8u * (nvb - b0))) - 1u;   // 1 .. 3 valid bytes
            q[j] = (q[j] & keep) | (fillv & ~keep);
        }
    }
}

}  // namespace

template <int PIX>
__global__ __launch_bounds__(kWencThreads, 4) void encode_window_kernel(WencParams p) {
    __shared__ __attribute__((aligned(16))) uint64_t s_pay[kWencPayWords + 1];   // + the trash word
    __shared__ uint32_t s_tot[kWencThreads / 64];
    __shared__ uint32_t s_chunk, s_ok, s_boot[2];
    __shared__ unsigned long long s_pre[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // Chunk ids as in enc16_kernel: a workgroup's first chunk is its arrival rank; static steps of G only when all G
    // workgroups have been seen running, tickets otherwise (or when forced).  One CAS decides for the whole launch.
    const uint32_t n_chunks = p.n_frames * p.chunks_per_frame, G = gridDim.x;
    if (tid == 0) {
        const uint32_t rank = atomicAdd(&p.ticket[0], 1u);
        uint32_t mode = n_chunks <= G ? 1u : 0u;   // one chunk per workgroup at most: nothing to agree on
        const uint64_t t0 = wall_clock64();
        while (!mode) {
            mode = __hip_atomic_load(&p.ticket[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (mode) break;
            const uint32_t arrived = __hip_atomic_load(&p.ticket[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (arrived >= G && !p.force_tickets) atomicCAS(&p.ticket[1], 0u, 1u);
            else if (p.force_tickets || wall_clock64() - t0 > 2000ull) atomicCAS(&p.ticket[1], 0u, 2u);
            else __builtin_amdgcn_s_sleep(2);
        }
        s_boot[0] = rank; s_boot[1] = mode;
    }
    __syncthreads();
    const bool static_mode = __builtin_amdgcn_readfirstlane(s_boot[1]) == 1u;
    uint32_t c = __builtin_amdgcn_readfirstlane(s_boot[0]);
    const uint64_t meta = 32ull + (uint64_t)(1 + PIX) * p.T;
    while (c < n_chunks) {
        const uint32_t f = c / p.chunks_per_frame, cf = c - f * p.chunks_per_frame;
        const uint32_t unit = cf * kWencThreads + tid;
        const bool has = unit < p.units;
        const uint32_t u = has ? unit : 0u;
        const uint32_t ty = u / p.lanes_per_row, ux = u - ty * p.lanes_per_row;
        const uint32_t tA = PIX == 1 ? ty * p.w + 2u * ux : u;          // the unit's first tile, stream order
        const bool hasB = PIX == 1 && has && 2u * ux + 1u < p.w;
        const uint32_t cx = (PIX == 1 ? 16u : 8u) * ux;                  // the unit's first window column
        int ox = p.x0, oy = p.y0;
        if (p.origins) {   // a tracker's moving window, clamped into the source as dbde_hip_decode_roi clamps
            ox = p.origins[2u * f];
            oy = p.origins[2u * f + 1u];
            ox = ox < 0 ? 0 : (ox > p.W - p.rw ? p.W - p.rw : ox);
            oy = oy < 0 ? 0 : (oy > p.H - p.rh ? p.H - p.rh : oy);
        }
        // ---- the fetch: 8 rows x 16 bytes.  Source offsets are 64-bit.
        uint32_t q[8][4];
        const uint32_t nvb = ((uint32_t)p.rw - cx) * (uint32_t)PIX < 16u ? ((uint32_t)p.rw - cx) * (uint32_t)PIX : 16u;
        const uint32_t ylast = 8u * ty + 7u < (uint32_t)p.rh - 1u ? 8u * ty + 7u : (uint32_t)p.rh - 1u;
        const uint64_t col0 = (uint64_t)f * p.frame_stride + ((uint64_t)(uint32_t)ox + cx) * (uint64_t)PIX;
        const bool wide = !p.narrow && col0 + ((uint64_t)(uint32_t)oy + ylast) * p.pitch + 16ull <= p.image_bytes;
        if (has && wide) {
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint32_t yy = 8u * ty + (uint32_t)r < (uint32_t)p.rh - 1u ? 8u * ty + (uint32_t)r : (uint32_t)p.rh - 1u;
                const uint8_t *src = p.images + col0 + ((uint64_t)(uint32_t)oy + yy) * p.pitch;
                const u32x4_t x = __builtin_nontemporal_load(reinterpret_cast<const u32x4_unaligned *>(src));
                q[r][0] = x[0]; q[r][1] = x[1]; q[r][2] = x[2]; q[r][3] = x[3];
            }
            if (nvb < 16u) {   // the unit crosses the window's right edge
#pragma unroll
                for (int r = 0; r < 8; r++) extend_row<PIX>(q[r], nvb);
            }
        } else if (has) {   // the end of the readable extent is within 16 bytes, or a narrow window: valid bytes one by one
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint32_t yy = 8u * ty + (uint32_t)r < (uint32_t)p.rh - 1u ? 8u * ty + (uint32_t)r : (uint32_t)p.rh - 1u;
                const uint8_t *src = p.images + col0 + ((uint64_t)(uint32_t)oy + yy) * p.pitch;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    uint32_t wv = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const uint32_t bi = 4u * (uint32_t)j + (uint32_t)b;
                        const uint32_t a = bi < nvb ? bi : (PIX == 1 ? nvb - 1u : nvb - 2u + (bi & 1u));
                        wv |= (uint32_t)src[a] << (8 * b);
                    }
                    q[r][j] = wv;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) { q[r][0] = 0; q[r][1] = 0; q[r][2] = 0; q[r][3] = 0; }
        }
        // ---- depths, the chunk's word count
        uint32_t va[PIX == 1 ? 16 : 32], vb[16];
        uint32_t mnA, mxA, mnB = 0, mxB = 0, dA, dB = 0;
        if constexpr (PIX == 1) {
#pragma unroll
            for (int r = 0; r < 8; r++) { va[2 * r] = q[r][0]; va[2 * r + 1] = q[r][1]; vb[2 * r] = q[r][2]; vb[2 * r + 1] = q[r][3]; }
            tile_minmax(va, mnA, mxA);
            tile_minmax(vb, mnB, mxB);
            dA = has ? depth_of_range(mxA - mnA) : 0u;
            dB = hasB ? depth_of_range(mxB - mnB) : 0u;
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) { va[4 * r] = q[r][0]; va[4 * r + 1] = q[r][1]; va[4 * r + 2] = q[r][2]; va[4 * r + 3] = q[r][3]; }
            tile_minmax_u16(va, mnA, mxA);
            dA = has ? depth_of_range(mxA - mnA) : 0u;
        }
        const uint32_t dsum = dA + dB;
        const uint32_t incl = wave_scan_incl(dsum);
        if (lane == 63u) s_tot[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0, total = 0;
        for (uint32_t i = 0; i < kWencThreads / 64; i++) { wbase += i < wave ? s_tot[i] : 0u; total += s_tot[i]; }
        if (tid == 0) __hip_atomic_store(&p.state[c], kReady | (u64a)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

        // pack while the record travels (total <= kWencPayWords: the image holds every chunk)
        if constexpr (PIX == 1) {
            pack_tile8(va, mnA, dA, s_pay, wbase + incl - dsum);
            pack_tile8(vb, mnB, dB, s_pay, wbase + incl - dB);
        } else {
            pack_tile16w(va, mnA, dA, s_pay, wbase + incl - dsum);
        }

        // Prefix inside the frame and the frame's base without a serial chain (enc16_kernel): A = the chunks in front of
        // this one in its group of 64, B = the frame's groups in front, C / D = the same two levels over frame word counts
        // (concatenated layout).  A chunk that publishes a higher-level record does so before it waits for that level.
        if (wave == 0) {
            const uint64_t t_start = wall_clock64();
            const uint32_t g = cf >> 6, nA = cf & 63u, gpf = (p.chunks_per_frame + 63u) >> 6;
            const bool concat = p.slot_stride == 0ull;
            const uint32_t nC = concat ? (f & 63u) : 0u, fg = concat ? (f >> 6) : 0u;
            const u64a *rA = p.state + (size_t)f * p.chunks_per_frame + (size_t)g * 64u;
            const u64a *rB = p.gsum + (size_t)f * gpf;
            const u64a *rC = p.fsize + (size_t)(f & ~63u);
            uint64_t sA = 0, sB = 0, sC = 0, sD = 0, z0, z1, z2;
            uint32_t ok = 1u;
            const uint32_t nB = g < 64u ? g : 64u, nD = fg < 64u ? fg : 64u;
            const bool pub_group = nA == 63u, pub_frame = concat && cf == p.chunks_per_frame - 1u;
            if (!pub_group && !pub_frame) {
                ok = sum_records(rA, nA, rB, nB, rC, nC, p.fgsum, nD, lane, t_start, sA, sB, sC, sD);
            } else {
                ok = sum_records(rA, nA, rA, 0u, rA, 0u, rA, 0u, lane, t_start, sA, z0, z1, z2);
                if (pub_group && lane == 0 && ok)
                    __hip_atomic_store(&p.gsum[(size_t)f * gpf + g], kReady | (u64a)(sA + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (ok) ok = sum_records(rB, nB, rC, nC, rA, 0u, rA, 0u, lane, t_start, sB, sC, z0, z1);
            }
            for (uint32_t i = 64u; i < g && ok; i += 64u) {    // frames of more than 4096 chunks
                uint64_t x = 0;
                ok = sum_records(rB + i, g - i < 64u ? g - i : 64u, rA, 0u, rA, 0u, rA, 0u, lane, t_start, x, z0, z1, z2);
                sB += x;
            }
            const uint64_t inf = sA + sB, fwords = inf + total;
            if (pub_frame && lane == 0 && ok) {
                __hip_atomic_store(&p.fsize[f], kReady | (u64a)fwords, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (nC == 63u) __hip_atomic_store(&p.fgsum[fg], kReady | (u64a)(sC + fwords), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if ((pub_group || pub_frame) && ok) ok = sum_records(p.fgsum, nD, rA, 0u, rA, 0u, rA, 0u, lane, t_start, sD, z0, z1, z2);
            for (uint32_t i = 64u; i < fg && ok; i += 64u) {   // launches of more than 4096 frames
                uint64_t x = 0;
                ok = sum_records(p.fgsum + i, fg - i < 64u ? fg - i : 64u, rA, 0u, rA, 0u, rA, 0u, lane, t_start, x, z0, z1, z2);
                sD += x;
            }
            if (lane == 0) {
                s_pre[0] = inf;
                s_pre[1] = concat ? (uint64_t)f * meta + 8ull * (sC + sD) : (uint64_t)f * p.slot_stride;
                s_ok = ok;
                if (!ok) atomicOr(p.sticky, 1u);
            }
        }
        __syncthreads();
        if (!s_ok) return;
        const uint64_t inf = s_pre[0];
        uint8_t *fb = p.out + s_pre[1];
        if (has) {   // metadata of this lane's tiles
            fb[24 + tA] = (uint8_t)dA;
            uint8_t *m = fb + 28 + p.T + (uint64_t)PIX * tA;
            m[0] = (uint8_t)mnA;
            if (PIX == 2) m[1] = (uint8_t)(mnA >> 8);
            if (hasB) { fb[25 + tA] = (uint8_t)dB; m[1] = (uint8_t)mnB; }
        }
        copy_out(s_pay, fb + meta + 8ull * inf, total, tid);   // the chunk's contiguous payload
        if (tid == 0) {
            if (cf == 0u) {   // frame header and the first I32 fields (elapsed travels as an F64)
                const uint64_t index = p.indices ? p.indices[f] : p.first_index + f;
                const uint64_t el = p.elapsed_ns ? p.elapsed_ns[f] : 0ull;
                store_u32_bytes(fb, 2u);
                store_u64_any(fb + 4, index);
                store_u64_any(fb + 12, (uint64_t)__double_as_longlong(__ull2double_rn(el)));
                store_u32_bytes(fb + 20, p.T);
                store_u32_bytes(fb + 24 + p.T, (uint32_t)PIX * p.T);
                if (p.frame_offsets) p.frame_offsets[f] = s_pre[1];
            }
            if (cf == p.chunks_per_frame - 1u) {   // the frame's word count is known here
                const uint64_t words = inf + total;
                store_u32_bytes(fb + meta - 4ull, (uint32_t)words);
                if (p.frame_bytes) p.frame_bytes[f] = meta + 8ull * words;
            }
        }
        // the next chunk; the barrier also hands the LDS image back
        if (!static_mode && tid == 0) s_chunk = atomicAdd(&p.ticket[0], 1u);
        __syncthreads();
        c = static_mode ? c + G : __builtin_amdgcn_readfirstlane(s_chunk);
    }
}

int wenc_blocks_per_cu(uint32_t pix) {
    int n = 0;
    const hipError_t e = pix == 2u ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, encode_window_kernel<2>, kWencThreads, 0)
                                   : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, encode_window_kernel<1>, kWencThreads, 0);
    if (e != hipSuccess || n < 1) n = 1;
    return n < (int)kWencBlocksPerCu ? n : (int)kWencBlocksPerCu;
}

hipError_t launch_encode_window(const WencParams &p, uint32_t pix, uint32_t resident_blocks, hipStream_t s) {
    const uint32_t n_chunks = p.n_frames * p.chunks_per_frame;
    const dim3 grid(n_chunks < resident_blocks ? n_chunks : resident_blocks);
    if (pix == 2u) hipLaunchKernelGGL(encode_window_kernel<2>, grid, dim3(kWencThreads), 0, s, p);
    else hipLaunchKernelGGL(encode_window_kernel<1>, grid, dim3(kWencThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
