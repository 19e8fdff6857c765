// Device pieces that the conv kernel families share (gfx950): counted waits, compile-time loops, the MFMA step per element
// type, the 8-channel store of an epilogue.  Included after common.h by the conv_*.hip files.  What differs between the families --
// how their K loops feed the MFMAs -- stays in their own files.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

// operands of __builtin_amdgcn_global_load_lds (LDS-DMA): a global source, an LDS destination
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

// s_waitcnt vmcnt(N): at most N of this wave's vector-memory loads (LDS-DMA pieces included) still in flight; they retire in order
template <int N>
__device__ __forceinline__ void y3_wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N - 1>{}): a loop whose index is a compile-time
// constant inside the body (`decltype(i)::value`)
template <int... I, typename F>
__device__ __forceinline__ void y3_static_for_impl(std::integer_sequence<int, I...>, F &&f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void y3_static_for(F &&f) { y3_static_for_impl(std::make_integer_sequence<int, N>{}, f); }

// y3_wait_vmcnt<N>() that NAMES the registers it waits for -- 2, 4 or 2 x 2 of them, the destinations of inline-asm loads,
// which the compiler cannot see in flight.  The tie is what keeps the compiler from moving the registers' uses above the
// wait, and from re-using them while the load is in flight (a late load then overwrites whatever was put there:
// profiles/r05s_halo_dw.txt).  (One asm statement per count: asm operands take no pack expansion.)
template <int N, typename V>
__device__ __forceinline__ void y3_wait_vmcnt_for(V (&w)[2]) {
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(w[0]), "+v"(w[1]) : "n"(N) : "memory");
}
template <int N, typename V>
__device__ __forceinline__ void y3_wait_vmcnt_for(V (&w)[4]) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]) : "n"(N) : "memory");
}
template <int N, typename V>
__device__ __forceinline__ void y3_wait_vmcnt_for(V (&w)[2][2]) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(w[0][0]), "+v"(w[0][1]), "+v"(w[1][0]), "+v"(w[1][1]) : "n"(N) : "memory");
}

// acc += W (16 rows) * X (16 columns) over one 64-byte K-half; operands as the 16 raw bytes a lane holds
template <typename T>
struct Mma {
  // 16-bit element types (bf16, IEEE half): 32 k values, a lane's 16-byte chunk = 8 of them; one v_mfma_f32_16x16x32
  static __device__ __forceinline__ void run(f32x4 &acc, const u32x4 &w, const u32x4 &x) { acc = y3_mfma16<T>(w, x, acc); }
};
template <>
struct Mma<float> {
  // 16 floats; lane (r, q) holds floats 4q..4q+3 of row r.  MFMA j consumes element j of every lane: it sums k in
  // {j, 4+j, 8+j, 12+j}; the same permutation is applied to both operands, so the four MFMAs cover the K-half.
  static __device__ __forceinline__ void run(f32x4 &acc, const u32x4 &w, const u32x4 &x) {
    const f32x4 wf = __builtin_bit_cast(f32x4, w), xf = __builtin_bit_cast(f32x4, x);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[j], xf[j], acc, 0, 0, 0);
  }
};

// The last step of an epilogue for eight consecutive channels of one pixel (all eight valid): v[0..7] rounded to the storage
// type at op, one 16-byte store (16-bit modes) or two (float32).  The address is computed BEFORE the rounding; a site that writes
// `*address = y3_pack8<T>(v)` with the address expression on the left computes it after, and keeps that spelling (same bits,
// but another instruction order: profiles/r16_conv_device_code_compare.txt).
template <typename T>
__device__ __forceinline__ void y3_store8(T *op, const float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    *reinterpret_cast<u32x4 *>(op) = y3_pack8<T>(v);
  } else {
    *reinterpret_cast<f32x4 *>(op) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4 *>(op + 4) = f32x4{v[4], v[5], v[6], v[7]};
  }
}
