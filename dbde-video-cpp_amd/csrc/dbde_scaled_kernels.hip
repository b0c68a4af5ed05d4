// dbde_scaled_kernels.hip -- scaled float decode for MI355X (gfx950, wave64): the rw x rh window of each frame as
// v = ((float)p - D) * G in F32, F16 or BF16, straight from the compressed bytes (no integer image is written).
//
// decode_scaled_kernel<THREADS, PIX, OUT>: PIX = 1 for DBDE frames (U8 pixels), PIX = 2 for DBDE16 frames (U16 pixels);
// OUT = kScaledF32 / kScaledF16 / kScaledBF16.  One workgroup per (frame, window tile row, piece of THREADS tiles), one
// tile per thread.  Steps 1-3 are decode_roi_kernel's (dbde_roi_kernels.hip), repeated here so that the window decoder's
// listing stays as it is: the tiles' depth / minimum bytes and one block scan for the payload offsets, the piece's
// payload range into LDS as aligned 16-byte blocks, each tile cut into registers and then into an LDS band of 8 image
// rows that reuses the payload buffer.  The band stays in the pixel type: a float band would quadruple the LDS and cost
// the occupancy that hides the one dependent load chain.  Then
//   4. the window's part of the band leaves as ONE contiguous output range when the piece spans the whole window width,
//      row by row otherwise; one thread per aligned 16-byte block of the OUTPUT (4 F32 or 8 F16 / BF16 elements).  A
//      whole block inside one window row reads its pixels from the band as dwords and its D and G as 16-byte loads
//      that are told of their 4-byte alignment; a block that a window row ends in, and the range's first and last
//      partial block, go element by element.  (p - D) * G is two IEEE binary32 operations (a subtraction feeding a
//      multiplication is not a contractible pattern), the result is rounded once, to nearest even, by v_cvt_pk_f16_f32 /
//      v_cvt_pk_bf16_f32, and a whole block is one nontemporal 16-byte store.  The maps are indexed by FRAME coordinates
//      and read with the default cache policy: every frame reads them again.  A NULL map is a wave-uniform branch to
//      the scalar: nothing is loaded.
// Latency is hidden by occupancy, as in decode_roi_kernel.
#include "dbde_scaled_kernels.h"

#include <type_traits>

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));   // native vector for the nontemporal builtins
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_a4_t __attribute__((ext_vector_type(4), aligned(4)));   // four map entries: 4-byte aligned only
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

template <uint32_t OUT> struct ElemOf { typedef float type; };
template <> struct ElemOf<kScaledF16> { typedef _Float16 type; };
template <> struct ElemOf<kScaledBF16> { typedef __bf16 type; };

// N consecutive map entries from m + idx, or the scalar when there is no map (uniform: p.dark / p.gain).
template <uint32_t N>
__device__ __forceinline__ void load_map(const float *m, size_t idx, float s, float (&o)[N]) {
    if (m) {
#pragma unroll
        for (uint32_t k = 0; k < N; k += 4u) {
            const f32x4_a4_t t = *reinterpret_cast<const f32x4_a4_t *>(m + idx + k);
            o[k] = t.x; o[k + 1u] = t.y; o[k + 2u] = t.z; o[k + 3u] = t.w;
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < N; k++) o[k] = s;
    }
}

// The binary32 product as a value of its own.  Without it the compiler folds the multiplication into the F16
// conversion (v_fma_mixlo_f16: a * G + 0 rounded once), which rounds once where the contract rounds twice and turns a
// product of -0 into +0.
__device__ __forceinline__ float rounded32(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// Two values rounded to nearest even into one dword of two F16 / BF16 elements.
template <uint32_t OUT>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    a = rounded32(a);
    b = rounded32(b);
    f32x2_t v;
    v.x = a; v.y = b;
    if constexpr (OUT == kScaledF16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_t));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

}  // namespace

template <uint32_t THREADS, uint32_t PIX, uint32_t OUT>
__global__ __launch_bounds__(THREADS) void decode_scaled_kernel(ScaledParams sp) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    static_assert(OUT == kScaledF32 || OUT == kScaledF16 || OUT == kScaledBF16, "F32, F16 or BF16 output");
    typedef typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type Pix;
    typedef typename std::conditional<PIX == 1u, uint2, uint4>::type Row;   // one tile row of 8 pixels
    typedef typename ElemOf<OUT>::type Elem;
    constexpr uint32_t NW = THREADS / 64u;
    constexpr uint32_t kPayBytes = kScaledPayBytesOf(THREADS, PIX);
    constexpr uint32_t kPitch = THREADS * 8u;   // band row in pixels: THREADS tiles of 8 pixels
    __shared__ __attribute__((aligned(16))) uint32_t s_pay[kPayBytes / 4u];   // the payload, then the band
    static_assert(8u * PIX * kPitch + 4u <= kPayBytes, "the band must fit the payload buffer");
    const Pix *band = reinterpret_cast<const Pix *>(s_pay);
    __shared__ uint32_t s_wsum[2][NW];
    const RoiParams &p = sp.roi;

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

    // ---- 1. depth / minimum bytes, offsets (decode_roi_kernel's step 1) ----
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
        } else {   // the U16 minima start at 28 + T, possibly at an odd address: byte by byte
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

    // ---- 2. the piece's payload into LDS (decode_roi_kernel's step 2) ----
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

    // ---- 3. tile rows -> registers -> the band (decode_roi_kernel's step 3) ----
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

    // ---- 4. the window's part of the band -> (p - D) * G -> the output (in elements) ----
    constexpr uint32_t ES = kScaledElemBytesOf(OUT), NE = 16u / ES;   // bytes of an element, elements of a block
    constexpr uint32_t NP = NE * PIX / 4u;                            // dwords of a block's pixels
    const int px0 = 8 * (int)txp;                                       // first pixel column of the piece
    const int c_lo = px0 > x ? px0 : x;
    const int c_hi = px0 + 8 * (int)nt < x + p.rw ? px0 + 8 * (int)nt : x + p.rw;
    const int r_lo = 8 * (int)ty > y ? 8 * (int)ty : y;
    const int r_hi = 8 * (int)ty + 8 < y + p.rh ? 8 * (int)ty + 8 : y + p.rh;
    const uint32_t pw = (uint32_t)(c_hi - c_lo), nr = (uint32_t)(r_hi - r_lo);
    const uint32_t bx = (uint32_t)(c_lo - px0), by = (uint32_t)(r_lo - 8 * (int)ty);
    Elem *dst = reinterpret_cast<Elem *>(p.out) + (size_t)f * (size_t)p.rw * (size_t)p.rh + (size_t)(r_lo - y) * (size_t)p.rw +
                (size_t)(c_lo - x);
    const size_t m0 = (size_t)r_lo * (size_t)p.W + (size_t)c_lo;   // the maps' entry of the band's first window pixel
    const float *dark = sp.dark, *gain = sp.gain;
    const bool whole = pw == (uint32_t)p.rw;   // rows of the window are adjacent in the output: one range
    const uint32_t nseg = whole ? 1u : nr, len = whole ? nr * pw : pw;
    for (uint32_t sg = 0; sg < nseg; sg++) {
        Elem *g = dst + (size_t)sg * (size_t)p.rw;
        const uintptr_t g0 = reinterpret_cast<uintptr_t>(g), a0 = g0 & ~(uintptr_t)15, g1 = g0 + ES * len;
        const uint32_t nb = (uint32_t)((g1 - a0 + 15u) >> 4);
        for (uint32_t i = tid; i < nb; i += THREADS) {
            const uintptr_t ba = a0 + 16u * i;
            const uint32_t lo = ba < g0 ? (uint32_t)(g0 - ba) / ES : 0u;        // elements of the block inside the range
            const uint32_t hi = ba + 16u > g1 ? (uint32_t)(g1 - ba) / ES : NE;
            const uint32_t L = (uint32_t)(ba + ES * lo - g0) / ES;   // the first element's place in the range
            uint32_t row = sg, col = L;                              // (row, column) in the window's part of the band
            if (whole) { row = L / pw; col = L - row * pw; }         // one range of nr rows at pitch pw
            if (lo == 0u && hi == NE) {
                float pv[NE], D[NE], G[NE];
                if (col + NE <= pw) {   // the block lies inside one window row
                    const uint32_t a = PIX * ((by + row) * kPitch + bx + col);
#pragma unroll
                    for (uint32_t k = 0; k < NP; k++) {
                        const uint32_t w = lds_u32_at(s_pay, a + 4u * k);
                        if constexpr (PIX == 1u) {
                            pv[4u * k] = (float)(w & 0xFFu); pv[4u * k + 1u] = (float)((w >> 8) & 0xFFu);
                            pv[4u * k + 2u] = (float)((w >> 16) & 0xFFu); pv[4u * k + 3u] = (float)(w >> 24);
                        } else {
                            pv[2u * k] = (float)(w & 0xFFFFu); pv[2u * k + 1u] = (float)(w >> 16);
                        }
                    }
                    const size_t mi = m0 + (size_t)row * (size_t)p.W + col;
                    load_map<NE>(dark, mi, sp.dark0, D);
                    load_map<NE>(gain, mi, sp.gain0, G);
                } else {   // a window row ends inside the block
#pragma unroll
                    for (uint32_t k = 0; k < NE; k++) {
                        const size_t mi = m0 + (size_t)row * (size_t)p.W + col;
                        pv[k] = (float)band[(by + row) * kPitch + bx + col];
                        D[k] = dark ? dark[mi] : sp.dark0;
                        G[k] = gain ? gain[mi] : sp.gain0;
                        if (++col == pw) { col = 0; row++; }
                    }
                }
                u32x4_t o;
                if constexpr (OUT == kScaledF32) {
                    o.x = __float_as_uint((pv[0] - D[0]) * G[0]); o.y = __float_as_uint((pv[1] - D[1]) * G[1]);
                    o.z = __float_as_uint((pv[2] - D[2]) * G[2]); o.w = __float_as_uint((pv[3] - D[3]) * G[3]);
                } else {
                    o.x = pack2<OUT>((pv[0] - D[0]) * G[0], (pv[1] - D[1]) * G[1]);
                    o.y = pack2<OUT>((pv[2] - D[2]) * G[2], (pv[3] - D[3]) * G[3]);
                    o.z = pack2<OUT>((pv[4] - D[4]) * G[4], (pv[5] - D[5]) * G[5]);
                    o.w = pack2<OUT>((pv[6] - D[6]) * G[6], (pv[7] - D[7]) * G[7]);
                }
                __builtin_nontemporal_store(o, reinterpret_cast<u32x4_t *>(ba));   // the output is written once
            } else {   // the range's first / last block: the elements inside it only
                for (uint32_t b = lo; b < hi; b++) {
                    const size_t mi = m0 + (size_t)row * (size_t)p.W + col;
                    const float v = ((float)band[(by + row) * kPitch + bx + col] - (dark ? dark[mi] : sp.dark0)) *
                                    (gain ? gain[mi] : sp.gain0);
                    reinterpret_cast<Elem *>(ba)[b] = (Elem)rounded32(v);
                    if (++col == pw) { col = 0; row++; }
                }
            }
        }
    }
}

namespace {

template <uint32_t THREADS, uint32_t PIX>
hipError_t launch_out(const ScaledParams &p, uint32_t grid, uint32_t out, hipStream_t s) {
    if (out == kScaledF32) hipLaunchKernelGGL((decode_scaled_kernel<THREADS, PIX, kScaledF32>), dim3(grid), dim3(THREADS), 0, s, p);
    else if (out == kScaledF16) hipLaunchKernelGGL((decode_scaled_kernel<THREADS, PIX, kScaledF16>), dim3(grid), dim3(THREADS), 0, s, p);
    else hipLaunchKernelGGL((decode_scaled_kernel<THREADS, PIX, kScaledBF16>), dim3(grid), dim3(THREADS), 0, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_decode_scaled(const ScaledParams &p, uint32_t n_frames, uint32_t threads, uint32_t pix, uint32_t out,
                                hipStream_t s) {
    if ((pix != 1u && pix != 2u) || out > kScaledBF16 ||
        (threads != kScaledNarrowThreads && threads != kScaledWideThreadsOf(pix)))
        return hipErrorInvalidValue;
    const uint32_t grid = n_frames * p.roi.rows * p.roi.pieces;   // (the host keeps it below 2^31)
    if (pix == 1u)
        return threads == kScaledNarrowThreads ? launch_out<kScaledNarrowThreads, 1>(p, grid, out, s)
                                               : launch_out<kScaledWideThreadsOf(1), 1>(p, grid, out, s);
    return threads == kScaledNarrowThreads ? launch_out<kScaledNarrowThreads, 2>(p, grid, out, s)
                                           : launch_out<kScaledWideThreadsOf(2), 2>(p, grid, out, s);
}

}  // namespace dbde
