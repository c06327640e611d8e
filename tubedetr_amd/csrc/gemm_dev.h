// Device helpers the GEMM-shaped kernel files share (gemm_conv.hip: forward / input-gradient GEMMs; conv_wgrad.hip: weight gradients; the
// bf16 pair packing also stem.hip and bottleneck.hip): MFMA wrappers per element type, 8 / 16-byte packing and unpacking, non-temporal
// 16-byte loads / stores, the inline-asm LDS fragment read and the counted wait.  Each declared here once.
#pragma once
#include <type_traits>

#include "td_common.h"

namespace td {

template <typename T>
struct Mfma;
template <>
struct Mfma<u16> {
  static __device__ __forceinline__ void run(const uint4& wf, const uint4& af, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)&wf, *(const bf16x8*)&af, acc, 0, 0, 0);
  }
};
template <>
struct Mfma<float> {
  // 16 fp32 of K per lane-group row chunk: lane (i, g) holds k = 4g..4g+3; MFMA step s consumes element s
  // of both operands (same k permutation on both sides, the dot product is unchanged).
  static __device__ __forceinline__ void run(const uint4& wf, const uint4& af, f32x4& acc) {
    const float* a = (const float*)&wf;
    const float* b = (const float*)&af;
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
  }
};

template <typename T>
__device__ __forceinline__ void load4(const char* base, size_t off, float (&o)[4]);
template <>
__device__ __forceinline__ void load4<float>(const char* base, size_t off, float (&o)[4]) {
  float4 v = *(const float4*)(base + off * 4);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
template <>
__device__ __forceinline__ void load4<u16>(const char* base, size_t off, float (&o)[4]) {
  uint2 v = *(const uint2*)(base + off * 2);
  o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
  o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
}
template <typename T, typename V>
__device__ __forceinline__ void unpack4(const V& v, float (&o)[4]);
template <>
__device__ __forceinline__ void unpack4<float, float4>(const float4& v, float (&o)[4]) {
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
template <>
__device__ __forceinline__ void unpack4<u16, uint2>(const uint2& v, float (&o)[4]) {
  o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
  o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
}
// 16 bytes of T <-> floats (8 bf16 or 4 fp32); bf16 packing uses the gfx950 v_cvt_pk_bf16_f32 (round-to-nearest-even)
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  bf16x2_t v = {(__bf16)lo, (__bf16)hi};
  return *(uint32_t*)&v;
}
// ReLU of two packed bf16: as 16-bit integers, max(x, 0) (v_pk_max_i16) - a negative value (sign bit set, -0.0 included) becomes +0.0,
// a non-negative one is unchanged.  ONE operation per two values behind the conversion; fmaxf(x, 0.f) before it is two per value
// (the compiler quiets a possible signalling NaN with a v_max x, x first).
// (As asm: written with vector types the compiler splits the conversion in front of it into two half conversions and a v_perm.  The
// CONVERSION must stay the compiler's own instruction: it is the first reader of an MFMA result, and the wait states an MFMA -> VALU
// read needs are inserted by the compiler's hazard pass, which does not look into asm operands - a v_cvt_pk_bf16_f32 written as
// asm read accumulators the matrix pipe had not written yet.)
__device__ __forceinline__ uint32_t relu_bf16x2(uint32_t v) {
  uint32_t r;
  asm("v_pk_max_i16 %0, %1, 0" : "=v"(r) : "v"(v));
  return r;
}
template <typename T>
__device__ __forceinline__ void unpack16(const uint4& v, float (&o)[16 / sizeof(T)]);
template <>
__device__ __forceinline__ void unpack16<float>(const uint4& v, float (&o)[4]) {
  o[0] = __uint_as_float(v.x); o[1] = __uint_as_float(v.y); o[2] = __uint_as_float(v.z); o[3] = __uint_as_float(v.w);
}
template <>
__device__ __forceinline__ void unpack16<u16>(const uint4& v, float (&o)[8]) {
  o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
  o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  o[4] = __uint_as_float(v.z << 16); o[5] = __uint_as_float(v.z & 0xffff0000u);
  o[6] = __uint_as_float(v.w << 16); o[7] = __uint_as_float(v.w & 0xffff0000u);
}
template <typename T>
__device__ __forceinline__ uint4 pack16(const float (&v)[16 / sizeof(T)]);
template <>
__device__ __forceinline__ uint4 pack16<float>(const float (&v)[4]) {
  return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
}
template <>
__device__ __forceinline__ uint4 pack16<u16>(const float (&v)[8]) {
  return make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
}
template <typename T>
__device__ __forceinline__ void store4(char* base, size_t off, const float (&v)[4]);
template <>
__device__ __forceinline__ void store4<float>(char* base, size_t off, const float (&v)[4]) {
  *(float4*)(base + off * 4) = make_float4(v[0], v[1], v[2], v[3]);
}
template <>
__device__ __forceinline__ void store4<u16>(char* base, size_t off, const float (&v)[4]) {
  uint2 o;
  o.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
  o.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
  *(uint2*)(base + off * 2) = o;
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// 16-byte epilogue operand loads / result stores, non-temporal (TD_NT bit 0: loads, bit 1: stores; 0 = plain, for A/B builds):
// these tensors are 0.1 - 1 GB streams that are touched once per launch; measured on the K >= 512 pointwise launches
// -12 .. -18 %, on the persistent 1x1 instance 5.05 -> 5.41 TB/s.
#ifndef TD_NT
#define TD_NT 3
#endif
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 ld16(const char* p) {
#if TD_NT & 1
  const u32x4_t v = __builtin_nontemporal_load((const u32x4_t*)p);
  return make_uint4(v.x, v.y, v.z, v.w);
#else
  return *(const uint4*)p;
#endif
}
__device__ __forceinline__ void st16(char* p, const uint4& v) {
#if TD_NT & 2
  __builtin_nontemporal_store(u32x4_t{v.x, v.y, v.z, v.w}, (u32x4_t*)p);
#else
  *(uint4*)p = v;
#endif
}

// fragment reads and counted waits of the kernels that order their LDS-DMA by hand (conv_gemm_big8_kernel's comment has the rules)
#ifndef TD_ABL
#define TD_ABL 0  // timing ablations of conv_gemm_big8_kernel (tools/build_variant.sh; results are WRONG with any bit set): 1 (was: no K walk), 2 no DMA, 4 no fragment reads, 8 no s_setprio, 16 stage buffers pre-filled with pseudo-random values (with 2: MFMAs on toggling operands without any L2 -> LDS traffic), 32 activation pieces of taps 1.. out of range
#endif
template <int OFF>
__device__ __forceinline__ u32x4_t lds_read16(uint32_t addr) {
  u32x4_t r;
#if TD_ABL & 4
  asm volatile("" : "=v"(r) : "v"(addr));
#else
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
#endif
  return r;
}
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int I>
using ic = std::integral_constant<int, I>;

}  // namespace td
