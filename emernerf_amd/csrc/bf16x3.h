// bf16x3: fp32-equivalent products on the bf16 matrix pipe of gfx950.  Each fp32 value is split exactly into three bf16
// terms and a product is the six partial products of order <= 2^-16, smallest first, accumulated in fp32 (csrc/mlp_fused.hip
// has the error argument; tests/_head_probe.py emulates exactly this split).  Shared by csrc/mlp.hip and csrc/mlp_fused.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace emer {

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using s16x4 = __attribute__((ext_vector_type(4))) short;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

__device__ __forceinline__ unsigned pk_bf16(float a, float b) {  // v_cvt_pk_bf16_f32 (round to nearest even)
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
// (a, b) -> packed bf16 pairs h, m, l with a = a_h + a_m + a_l (+ <= 2^-24 |a|); both subtractions are exact
__device__ __forceinline__ void split3(float a, float b, unsigned &h, unsigned &m, unsigned &l) {
    h = pk_bf16(a, b);
    const float ra = a - __uint_as_float(h << 16), rb = b - __uint_as_float(h & 0xffff0000u);
    m = pk_bf16(ra, rb);
    const float sa = ra - __uint_as_float(m << 16), sb = rb - __uint_as_float(m & 0xffff0000u);
    l = pk_bf16(sa, sb);
}

// K = 32 and 32 x 32 x 16: A, B u32x4 (eight packed bf16); 16 x 16 x 16: u32x2 (four).  C: f32x4 (16 x 16) or f32x16 (32 x 32)
#define EMER_MF(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, B), C, 0, 0, 0)
#define EMER_MF16(A, B, C) __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, A), __builtin_bit_cast(s16x4, B), C, 0, 0, 0)
#define EMER_MF32(A, B, C) __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, B), C, 0, 0, 0)

}  // namespace emer
