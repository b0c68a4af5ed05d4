// dbde_device.h -- device helpers shared by the kernel files (gfx950, wave64; device code only).
//
// encode_kernel / decode_kernel use wave_scan_incl and wave_sum, but bench.kernels_fingerprint() hashes only
// dbde_kernels.hip / .h and dbde_bits.h: after an edit here, profiles/listing_diff.py shows whether the kernels that
// profiles/hbm_traffic.json describes are still the measured ones.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dbde {

// Wave-wide inclusive scan with DPP row shifts / row broadcasts (gfx9 wave64 idiom): no LDS.
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x) {
    uint32_t t = x;
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x111, 0xF, 0xF, false);   // row_shr:1
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x112, 0xF, 0xF, false);   // row_shr:2
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x114, 0xF, 0xF, false);   // row_shr:4
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x118, 0xF, 0xF, false);   // row_shr:8
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1,3
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2,3
    return t;
}

// Sum over the wave, in every lane.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The four bytes at LDS byte address a (any alignment; the dword after the one holding a must be inside the array).
__device__ __forceinline__ uint32_t lds_u32_at(const uint32_t *s32, uint32_t a) {
    return __builtin_amdgcn_alignbyte(s32[(a >> 2) + 1u], s32[a >> 2], a & 3u);
}

// cut_row16's step: four pixels of d bits at bit 0 of the 64-bit window x1:x0 -> two dwords of two U16 pixels each,
// the minimum added.  c2 / c3: 2d >= 32 / 3d >= 32, the caller's per-tile flags.  The 16-bit projection kernel (one
// lane per half row) calls it on its own.
__device__ __forceinline__ void cut_four16(uint32_t x0, uint32_t x1, const uint32_t &d, const uint32_t &m32,
                                           const uint32_t &mn2, const bool &c2, const bool &c3, uint32_t &e0,
                                           uint32_t &e1) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const uint32_t p0 = x0 & m32;
    const uint32_t p1 = __builtin_amdgcn_alignbit(x1, x0, d) & m32;
    const uint32_t p2 = __builtin_amdgcn_alignbit(c2 ? 0u : x1, c2 ? x1 : x0, 2u * d) & m32;
    const uint32_t p3 = __builtin_amdgcn_alignbit(c3 ? 0u : x1, c3 ? x1 : x0, 3u * d) & m32;
    e0 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, p0 | (p1 << 16)) + __builtin_bit_cast(u16x2, mn2));
    e1 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, p2 | (p3 << 16)) + __builtin_bit_cast(u16x2, mn2));
}

// One DBDE16 tile row (8 pixels of d <= 16 bits, the 8d-bit integer at byte a of the tile payload) -> four dwords of two
// U16 pixels each; shared by dec16_kernel and decode_roi_kernel<T, 2>.  The row's two 4-pixel halves start at bytes a
// and ah = a + d/2 (plus 4 bits when d is odd); q / qh point at the three aligned dwords holding each.  A half comes out
// of its dwords with v_alignbyte, a pixel is one v_alignbit at i*d masked with m32 (the low d bits; shift counts are
// taken modulo 32: from 32 on, the half's high dword is shifted instead), and the minimum (mn2: in both 16-bit lanes) is
// added modulo 2^16 with v_pk_add_u16, as the format says.  d, m32 and mn2 are the caller's per-tile values, taken by
// reference as the kernels' own lambdas captured them: passed by value, the compiler orders the kernels' first loads
// differently.
__device__ __forceinline__ void cut_row16(const uint32_t *q, const uint32_t *qh, uint32_t a, uint32_t ah, const uint32_t &d,
                                          const uint32_t &m32, const uint32_t &mn2, uint32_t &o0, uint32_t &o1,
                                          uint32_t &o2, uint32_t &o3) {
    const uint32_t sh_odd = (d & 1u) * 4u;
    const bool c2 = 2u * d >= 32u, c3 = 3u * d >= 32u;
    const uint32_t x0 = __builtin_amdgcn_alignbyte(q[1], q[0], a), x1 = __builtin_amdgcn_alignbyte(q[2], q[1], a);
    const uint32_t w0 = __builtin_amdgcn_alignbyte(qh[1], qh[0], ah), w1 = __builtin_amdgcn_alignbyte(qh[2], qh[1], ah);
    const uint32_t h0 = __builtin_amdgcn_alignbit(w1, w0, sh_odd), h1 = w1 >> sh_odd;
    cut_four16(x0, x1, d, m32, mn2, c2, c3, o0, o1);
    cut_four16(h0, h1, d, m32, mn2, c2, c3, o2, o3);
}

// The packing half of a DBDE16 tile row, shared by enc16_kernel and the crop's re-pack: four pixels (two dwords, 16 bits
// each, already minus the minimum) -> the 4*d-bit integer p0 | p1<<d | p2<<2d | p3<<3d.
__device__ __forceinline__ uint64_t pack_four16(uint32_t a, uint32_t b, uint32_t d) {
    const uint64_t lo = (uint64_t)(a & 0xFFFFu) | ((uint64_t)(a >> 16) << d);
    const uint64_t hi = (uint64_t)(b & 0xFFFFu) | ((uint64_t)(b >> 16) << d);
    return lo | (hi << (2u * d));
}

}  // namespace dbde
