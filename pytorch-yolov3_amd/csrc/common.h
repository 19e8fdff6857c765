// Shared device/host helpers for libyolov3_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>

#include <mutex>
#include <type_traits>

#include "yolov3_hip.h"

typedef __bf16 bf16_t;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16_t;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

#define Y3_WAVE 64
// cache policy of the LDS-DMA loads (the builtin's last argument: gfx940+ CPol bits, 1 = sc0, 2 = nt, 16 = sc1): 0 in the
// product; experiment builds set them per operand (`make variant FLAGS="-DY3_AUX_W=2"`: weight tiles non-temporal, i.e. past L1)
#ifndef Y3_AUX_W
#define Y3_AUX_W 0
#endif
#ifndef Y3_AUX_A
#define Y3_AUX_A 0
#endif
#ifndef Y3_AUX_H
#define Y3_AUX_H 0        // strip kernel: the halo (pixel) slices
#endif
#define Y3_LEAKY_SLOPE 0.1f

// diagnostic builds only (y3_set_tuning("debug", v)): 0 in the product.  The hook of timing experiments (a launcher passes it to its
// kernel as a flag bit); the experiments that read it are measured and removed (profiles/), so nothing reads it at present
int y3_debug_flags();
// CU count of the current device (api.hip); the choosers' grid-size heuristics scale with it
int y3_device_cus();

// thread-local error string shared by all translation units
void y3_set_error(const char *fmt, ...);

#define Y3_HIP_CHECK(expr)                                                               \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      y3_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return Y3_ERR_HIP;                                                                 \
    }                                                                                    \
  } while (0)

#define Y3_REQUIRE(cond, ...)     \
  do {                            \
    if (!(cond)) {                \
      y3_set_error(__VA_ARGS__);  \
      return Y3_ERR_INVALID;      \
    }                             \
  } while (0)

// Every kernel of the library is launched through Y3_LAUNCH.  Normally that is hipLaunchKernelGGL.  Inside
// y3_plan_run_profiled (api.hip) the calling thread has a Y3KernelTimer set and the launch goes through
// hipExtLaunchKernelGGL with a start / stop event pair BOUND TO THE DISPATCH: their elapsed time is the kernel's own
// begin -> end on the device (the figure rocprofv3's kernel trace reports), without the ~5 us of dispatch and barrier-packet
// handling that an event recorded on the stream before and after a launch includes (y3_plan_run_timed).
struct Y3KernelTimer {
  hipEvent_t *start, *stop;
  int n, cap;
};
// The launch log (y3_debug_launch_log_begin / _end, api.hip): while the calling thread has one, Y3_LAUNCH appends the kernel's
// code-object symbol name -- the mangled name in the `.name` field of the AMDGPU metadata -- before it launches.  Host code
// only.  Timer and log share one thread-local pair, so a launch with neither pays the one thread-local access it always paid.
struct Y3LaunchLog;
struct Y3LaunchHooks {
  Y3KernelTimer *timer;
  Y3LaunchLog *log;
};
Y3LaunchHooks *y3_launch_hooks();
void y3_launch_log_append(Y3LaunchLog *log, const void *host_function, hipStream_t stream);
#define Y3_LAUNCH(kernel, grid, block, lds, stream, ...)                                                             \
  do {                                                                                                               \
    const Y3LaunchHooks *_hk = y3_launch_hooks();                                                                    \
    if (_hk->log) y3_launch_log_append(_hk->log, reinterpret_cast<const void *>(kernel), stream);                    \
    Y3KernelTimer *_kt = _hk->timer;                                                                                 \
    if (_kt && _kt->n < _kt->cap) {                                                                                  \
      hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, _kt->start[_kt->n], _kt->stop[_kt->n], 0, __VA_ARGS__); \
      ++_kt->n;                                                                                                      \
    } else {                                                                                                         \
      hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                             \
    }                                                                                                                \
  } while (0)

// What a launch is made of: workgroups (64-bit, so that plan creation can refuse a grid no launch holds), threads per workgroup,
// dynamic LDS bytes.  A chooser records them in its y3_step; the launcher launches exactly that.
struct y3_dims {
  long long grid = 0;
  int block = 0;
  size_t lds = 0;
};

// Launches one kernel instance through Y3_LAUNCH and checks the launch.  Dynamic LDS over 64 KiB needs the instance's limit
// raised first; the attribute is per device, so it is set on the instance's first such launch on each device (one lock and
// state per instance: the statics of this template).  Launches within 64 KiB take no lock.
template <auto Kernel, typename... A>
int y3_launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const A &...args) {
  if (lds > 64 * 1024) {
    static std::mutex mu;
    static bool done[32];
    int dev = 0;
    Y3_HIP_CHECK(hipGetDevice(&dev));
    Y3_REQUIRE(dev >= 0 && dev < 32, "device index %d out of range", dev);
    std::lock_guard<std::mutex> lock(mu);
    if (!done[dev]) {
      Y3_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024));
      done[dev] = true;
    }
  }
  Y3_LAUNCH(Kernel, grid, block, lds, s, args...);
  Y3_HIP_CHECK(hipGetLastError());
  return Y3_OK;
}
template <auto Kernel, typename... A>
int y3_launch(const y3_dims &d, hipStream_t s, const A &...args) {
  return y3_launch<Kernel>(dim3((unsigned)d.grid), dim3(d.block), d.lds, s, args...);
}

// The instantiated values of one template parameter of a kernel family: the chooser asks has(v), the launcher pick(v, f),
// which returns f(std::integral_constant<int, V>{}) for the listed V == v, and fails for any other v.  The instances are
// emitted into the code object in list order (bench.device_code_sha256 sees the order): reordering a list moves kernels.
template <int... V>
struct y3_ints {
  static constexpr bool has(int v) { return ((v == V) || ...); }
  template <typename F>
  static int pick(int v, F &&f) {
    int rc = Y3_OK;
    if ((... || (v == V && ((rc = f(std::integral_constant<int, V>{})), true)))) return rc;
    y3_set_error("no kernel instance for template value %d", v);
    return Y3_ERR_INVALID;
  }
};

// 16-bit storage modes (bf16, IEEE half): the same kernels, instantiated per element type
static inline bool y3_is16(int dtype) { return dtype == Y3_BF16 || dtype == Y3_F16; }
static inline int y3_elem_size(int dtype) { return y3_is16(dtype) ? 2 : 4; }
// kernel names carry the element type: Y3_KNAME(dtype, "conv_halo_ws_", "_256x128") -> "conv_halo_ws_bf16_256x128"
#define Y3_KNAME(dt, pre, post) ((dt) == Y3_BF16 ? pre "bf16" post : ((dt) == Y3_F16 ? pre "f16" post : pre "f32" post))
// host-side dispatch on the element type: f(T{}) with T = bf16_t / f16_t / float (a generic lambda: `using T = decltype(tag)`)
template <typename F>
static inline int y3_by_dtype(int dtype, F &&f) {
  if (dtype == Y3_BF16) return f(bf16_t{});
  if (dtype == Y3_F16) return f(f16_t{});
  return f(float{});
}
template <typename F>
static inline int y3_by_dtype16(int dtype, F &&f) {   // kernels that exist for the 16-bit modes only
  return dtype == Y3_F16 ? f(f16_t{}) : f(bf16_t{});
}
static inline int y3_ceil_div(int a, int b) { return (a + b - 1) / b; }
// A launch holds fewer than 2^32 threads (grid x block): plan creation refuses a step whose recorded launch (y3_step.dims) is past
// the limit (api.hip check_launch)
constexpr long long kY3MaxThreads = ((1ll << 32) - 1) / 256 * 256;
static inline long long y3_ceil_div64(long long a, long long b) { return (a + b - 1) / b; }
// n / d == (umulhi(n, mul) + n) >> sh for 0 <= n < 2^31 (round-up method, d >= 1)
static inline void y3_fast_div(uint32_t d, uint32_t &mul, uint32_t &sh) {
  if (d <= 1) { mul = 0; sh = 0; return; }
  sh = 0;
  while ((1u << sh) < d) ++sh;
  mul = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << sh) - d)) / d + 1);
}

// Workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MiB L2); give each
// XCD one contiguous run of logical tile ids so that neighbouring tiles (which share an input
// halo / weight panel) hit the same L2.  Bijective for any grid size.  Placement only affects
// speed, never results.
__device__ __forceinline__ int y3_xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

// Output-channel placement that makes a lane's accumulators of an MFMA fragment PAIR eight consecutive channels.
// v_mfma_f32_16x16x32 leaves lane (fr, fq) with rows 4 fq .. 4 fq + 3 of each 16-row fragment for column (pixel) fr.  If,
// inside every aligned block of 32 weight rows (fragments h = 0, 1), row h*16 + 4q + i carries channel 8q + 4h + i, the
// lane holds channels 8 fq .. 8 fq + 7 of its pixel after both fragments: one 16-byte LDS write (8-lane groups, no
// conflicts with the usual XOR swizzle or an odd multiple of 16 bytes as pixel pitch) instead of two 8-byte ones whose
// 16-lane groups hit every 128-byte bank window twice or four times (tools/lds_conflicts.py).  Which row of a
// fragment a channel occupies does not enter any sum: results are bit-identical.
__host__ __device__ __forceinline__ constexpr int y3_pair_perm(int j) {
  return (j & ~31) | (((j >> 2) & 3) << 3) | (((j >> 4) & 1) << 2) | (j & 3);
}

template <typename T>
__device__ __forceinline__ float y3_to_float(T v);
template <>
__device__ __forceinline__ float y3_to_float<float>(float v) { return v; }
template <>
__device__ __forceinline__ float y3_to_float<bf16_t>(bf16_t v) { return (float)v; }
template <>
__device__ __forceinline__ float y3_to_float<f16_t>(f16_t v) { return (float)v; }

template <typename T>
__device__ __forceinline__ T y3_from_float(float v);
template <>
__device__ __forceinline__ float y3_from_float<float>(float v) { return v; }
template <>
__device__ __forceinline__ bf16_t y3_from_float<bf16_t>(float v) { return (bf16_t)v; }
template <>
__device__ __forceinline__ f16_t y3_from_float<f16_t>(float v) { return (f16_t)v; }   // v_cvt_f16_f32: nearest even, like numpy / torch

// The two 16-bit element types behind one interface: 8- / 4-wide vectors, the MFMA that consumes them (both issue at the
// same rate on gfx950: 16 passes for 16x16x32), conversions.  float32 accumulation in both.
template <typename T>
struct H16;
template <>
struct H16<bf16_t> {
  typedef bf16x8 v8;
  typedef bf16x4 v4;
  static __device__ __forceinline__ f32x4 mfma(const v8 &w, const v8 &x, const f32x4 &acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x, acc, 0, 0, 0);
  }
};
template <>
struct H16<f16_t> {
  typedef f16x8 v8;
  typedef f16x4 v4;
  static __device__ __forceinline__ f32x4 mfma(const v8 &w, const v8 &x, const f32x4 &acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(w, x, acc, 0, 0, 0);
  }
};
// acc += W (16 rows x 32 k) * X (32 k x 16 columns); operands as the 16 raw bytes a lane holds
template <typename T>
__device__ __forceinline__ f32x4 y3_mfma16(const u32x4 &w, const u32x4 &x, const f32x4 &acc) {
  typedef typename H16<T>::v8 v8;
  return H16<T>::mfma(__builtin_bit_cast(v8, w), __builtin_bit_cast(v8, x), acc);
}
// eight consecutive stored elements (16 raw bytes) added to v[0..7]: the shortcut operand of a conv epilogue
template <typename T>
__device__ __forceinline__ void y3_add8(float (&v)[8], const u32x4 &raw) {
  const typename H16<T>::v8 r = __builtin_bit_cast(typename H16<T>::v8, raw);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] += (float)r[i];
}
template <typename T>
__device__ __forceinline__ void y3_unpack8(float (&v)[8], const u32x4 &raw) {
  const typename H16<T>::v8 r = __builtin_bit_cast(typename H16<T>::v8, raw);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)r[i];
}
// v[0..7] rounded to the storage type (nearest even), as the 16 bytes of one store
template <typename T>
__device__ __forceinline__ u32x4 y3_pack8(const float (&v)[8]) {
  typename H16<T>::v8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (T)v[i];
  return __builtin_bit_cast(u32x4, o);
}
template <typename T>
__device__ __forceinline__ u32x2 y3_pack4(float a, float b, float c, float d) {
  const typename H16<T>::v4 o = {(T)a, (T)b, (T)c, (T)d};
  return __builtin_bit_cast(u32x2, o);
}

// Conv epilogue arithmetic for eight consecutive output channels: acc * scale + bias, then the activation.  Written
// on 2-wide vectors so that hipcc emits v_pk_fma_f32 / v_pk_mul_f32, and with v_max_f32 spelled out: max(v, 0.1 v) is
// v > 0 ? v : 0.1 v bit for bit (both operands carry v's sign), one instruction instead of compare + select, and fmaxf
// would add a canonicalising v_max per value.  The epilogues are VALU-bound (MI355X: 4 cycles per instruction and
// wave, 64 values per lane and tile).
__device__ __forceinline__ float y3_vmax(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// Activation of a conv op, from its flags: a run-time value of the layer (uniform across the grid, so the branches on it
// below are scalar branches, and the leaky / linear arithmetic is the same instruction sequence as before mish existed)
// (mish and logistic, the codes >= Y3_ACT_MISH, share one scalar branch after the linear form: y3_bn_act8)
enum : int { Y3_ACT_LINEAR = 0, Y3_ACT_LEAKY = 1, Y3_ACT_MISH = 2, Y3_ACT_LOGISTIC = 3 };
__host__ __device__ __forceinline__ int y3_act(uint32_t flags) {
  return (flags & Y3_F_LOGISTIC) ? Y3_ACT_LOGISTIC
                                 : ((flags & Y3_F_MISH) ? Y3_ACT_MISH : ((flags & Y3_F_LEAKY) ? Y3_ACT_LEAKY : Y3_ACT_LINEAR));
}
// mish(x) = x tanh(softplus(x)) = x t / (t + 2) with n = e^x, t = n (n + 2) = (1 + n)^2 - 1: one v_exp_f32, one v_rcp_f32,
// a few FMAs.  Above 20 the ratio is 1 in float32 (mish(x) == x there), and from about 44 on t overflows and the ratio
// would be inf / inf: x is returned instead.
__device__ __forceinline__ float y3_mish(float x) {
  const float n = __expf(x);
  const float t = n * (n + 2.0f);
  const float y = x * t * __builtin_amdgcn_rcpf(t + 2.0f);
  return x > 20.0f ? x : y;
}
// logistic(x) = 1 / (1 + e^-x): one v_exp_f32, one v_rcp_f32.  Saturates without a select: from x ~ 17 on e^-x is below half an
// ulp of 1, so the denominator is 1 and the result exactly 1; below x ~ -88.7 (and at -inf) e^-x is inf and the result exactly 0.
// The fused head kernels apply this same function to their logits, so fused and two-kernel heads give the same bits.
__device__ __forceinline__ float y3_logistic(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// Mish or logistic (the codes >= Y3_ACT_MISH, behind the caller's one scalar branch) as ONE instruction sequence: both are an
// exponential and a reciprocal, so the choice is a few selects on a uniform condition rather than a second code path (which
// made an epilogue spill).  Mish: x * t * rcp(t + 2), y3_mish's operations; logistic: 1 * rcp(1 + e^-x), y3_logistic's bits
// (the product with 1 is exact).
__device__ __forceinline__ float y3_act_tail(float x, int act) {
#pragma clang fp contract(off)   // t + 2 stays an add, as the eight-value mish loop it replaces compiled (no fma)
  const bool lg = act == Y3_ACT_LOGISTIC;
  const float n = __expf(lg ? -x : x);
  const float t = n * (n + 2.0f);
  const float y = (lg ? 1.0f : x * t) * __builtin_amdgcn_rcpf(lg ? 1.0f + n : t + 2.0f);
  return !lg && x > 20.0f ? x : y;
}
// one value: the scalar epilogues (float32 kernels, stem kernels)
__device__ __forceinline__ float y3_act1(float t, int act) {
  if (act == Y3_ACT_MISH) return y3_mish(t);
  if (act == Y3_ACT_LOGISTIC) return y3_logistic(t);
  return act == Y3_ACT_LEAKY ? (t > 0.f ? t : Y3_LEAKY_SLOPE * t) : t;
}
// eight values, activation `act` (Y3_ACT_*).  Leaky / linear: a slope of 1 makes max(v, slope * v) the identity without a
// branch (phi copies of all eight values otherwise).  Mish and logistic run the linear form and then, behind one scalar branch
// per eight values, replace each value in place: the leaky / linear path keeps its instruction sequence and nothing of the
// mish / logistic arithmetic is live across it.
__device__ __forceinline__ void y3_act_tail8(float (&v)[8], int act) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = y3_act_tail(v[i], act);
}
__device__ __forceinline__ void y3_bn_act8(float (&v)[8], const f32x4 &lo, const f32x4 &hi, const f32x4 &sc_lo,
                                           const f32x4 &sc_hi, const f32x4 &bi_lo, const f32x4 &bi_hi, int act) {
  const float slope = act == Y3_ACT_LEAKY ? Y3_LEAKY_SLOPE : 1.0f;
  f32x2 t[4];
  t[0] = f32x2{lo[0], lo[1]} * f32x2{sc_lo[0], sc_lo[1]} + f32x2{bi_lo[0], bi_lo[1]};
  t[1] = f32x2{lo[2], lo[3]} * f32x2{sc_lo[2], sc_lo[3]} + f32x2{bi_lo[2], bi_lo[3]};
  t[2] = f32x2{hi[0], hi[1]} * f32x2{sc_hi[0], sc_hi[1]} + f32x2{bi_hi[0], bi_hi[1]};
  t[3] = f32x2{hi[2], hi[3]} * f32x2{sc_hi[2], sc_hi[3]} + f32x2{bi_hi[2], bi_hi[3]};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 s = t[i] * slope;
    v[2 * i] = y3_vmax(t[i][0], s[0]);
    v[2 * i + 1] = y3_vmax(t[i][1], s[1]);
  }
  if (act >= Y3_ACT_MISH) y3_act_tail8(v, act);
}

// y3_bn_act8 for ONE value, operation by operation (acc * scale + bias, max(t, slope * t), then the mish / logistic tail): a
// kernel's one-element form gives the bits of the eight-wide epilogue (conv_grouped.hip).  Kept next to it: change both.
__device__ __forceinline__ float y3_bn_act1(float acc, float sc, float bi, int act) {
  const float slope = act == Y3_ACT_LEAKY ? Y3_LEAKY_SLOPE : 1.0f;
  const float t = acc * sc + bi;
  float v = y3_vmax(t, t * slope);
  if (act >= Y3_ACT_MISH) v = y3_act_tail(v, act);
  return v;
}

// Diagnostic build only (-DY3_STAMPS, `make stamps`): per-workgroup phase timing with s_memtime.
// Lane 0 of wave 0 adds the cycle count of each phase into g_y3_stamps[phase]; slot 7 counts
// workgroups.  Never compiled into the shipped library.
#ifdef Y3_STAMPS
static __device__ unsigned long long g_y3_stamps[8];  // one copy per translation unit
__device__ __forceinline__ unsigned long long y3_now() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define Y3_STAMP_DECL                                \
  unsigned long long _st_acc[7] = {0, 0, 0, 0, 0, 0, 0}; \
  unsigned long long _st_prev = y3_now();
// accumulate in registers; nothing touches memory until the kernel's last instruction
#define Y3_STAMP(slot)                            \
  do {                                            \
    const unsigned long long _now = y3_now();     \
    _st_acc[slot] += _now - _st_prev;             \
    _st_prev = _now;                              \
  } while (0)
#define Y3_STAMP_COUNT()                                                         \
  do {                                                                           \
    if (threadIdx.x == 0) {                                                      \
      for (int _i = 0; _i < 7; ++_i) atomicAdd(&g_y3_stamps[_i], _st_acc[_i]);   \
      atomicAdd(&g_y3_stamps[7], 1ull);                                          \
    }                                                                            \
  } while (0)
// defines  extern "C" int NAME(unsigned long long out[8])  that reads + clears this unit's counters
#define Y3_STAMP_READER(NAME)                                                                        \
  extern "C" int NAME(unsigned long long *out8) {                                                    \
    if (hipDeviceSynchronize() != hipSuccess) return Y3_ERR_HIP;                                     \
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_y3_stamps), 64) != hipSuccess) return Y3_ERR_HIP;     \
    unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                           \
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_y3_stamps), zero, 64) != hipSuccess) return Y3_ERR_HIP;       \
    return Y3_OK;                                                                                    \
  }
#else
#define Y3_STAMP_READER(NAME)
#define Y3_STAMP_DECL
#define Y3_STAMP(slot) do {} while (0)
#define Y3_STAMP_COUNT() do {} while (0)
#endif

// Y3_STAMPS_CLOCK (diagnostic, `make stamps STAMP_FLAGS=-DY3_STAMPS_CLOCK`): no stamp inside the K loop; thread 0
// stamps s_memtime (shader cycles) and s_memrealtime (100 MHz) around it: slot 0 = loop cycles, slot 1 = loop time in
// 10 ns ticks (in-kernel clock = slot0 / slot1 * 100 MHz: MI355X_MICROARCH.md, DVFS give-back item 6), slot 2 =
// cycles before the loop, slot 3 = cycles after it
#if defined(Y3_STAMPS) && defined(Y3_STAMPS_CLOCK)
#undef Y3_STAMP
#define Y3_STAMP(slot) do {} while (0)
__device__ __forceinline__ unsigned long long y3_now_real() {
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define Y3_CLK_BEGIN() unsigned long long _clk_r0 = 0; do { const unsigned long long _n = y3_now(); _st_acc[2] = _n - _st_prev; _st_prev = _n; _clk_r0 = y3_now_real(); } while (0)
#define Y3_CLK_END() do { const unsigned long long _n = y3_now(); _st_acc[0] = _n - _st_prev; _st_prev = _n; _st_acc[1] = y3_now_real() - _clk_r0; } while (0)
#ifdef Y3_STAMPS_EPI
// ... and the pieces of the epilogue in slots 4-6 (thread 0: K loop end -> first barrier -> tile parked -> written out)
#define Y3_EPI(slot) do { const unsigned long long _n = y3_now(); _st_acc[slot] = _n - _st_prev; _st_prev = _n; } while (0)
#define Y3_CLK_TAIL() do { if (threadIdx.x == 0) { _st_acc[3] = y3_now() - _st_prev; for (int _i = 0; _i < 7; ++_i) atomicAdd(&g_y3_stamps[_i], _st_acc[_i]); atomicAdd(&g_y3_stamps[7], 1ull); } } while (0)
#else
// slots 4-6: the first round of workgroups (blockIdx < 256) on its own: cycles before the loop, count x 1000, cycles after it
#define Y3_EPI(slot) do {} while (0)
#define Y3_CLK_TAIL() do { if (threadIdx.x == 0) { _st_acc[3] = y3_now() - _st_prev; for (int _i = 0; _i < 4; ++_i) atomicAdd(&g_y3_stamps[_i], _st_acc[_i]); if (blockIdx.x < 256) { atomicAdd(&g_y3_stamps[4], _st_acc[2]); atomicAdd(&g_y3_stamps[5], 1000ull); atomicAdd(&g_y3_stamps[6], _st_acc[3]); } atomicAdd(&g_y3_stamps[7], 1ull); } } while (0)
#endif
#else
#define Y3_CLK_BEGIN() do {} while (0)
#define Y3_CLK_END() do {} while (0)
#define Y3_CLK_TAIL() do {} while (0)
#define Y3_EPI(slot) do {} while (0)
#endif

// Y3_STAMPS_FINE (diagnostic): the ping-pong kernel stamps the pieces of its K-step instead of its phases
#if defined(Y3_STAMPS) && defined(Y3_STAMPS_CLOCK)
#define Y3_FINE(slot) do {} while (0)
#define Y3_COARSE(slot) do {} while (0)
#elif defined(Y3_STAMPS) && defined(Y3_STAMPS_FINE)
#define Y3_FINE(slot) Y3_STAMP(slot)
#define Y3_COARSE(slot) do { _st_prev = y3_now(); } while (0)
#else
#define Y3_FINE(slot) do {} while (0)
#define Y3_COARSE(slot) Y3_STAMP(slot)
#endif

// ---- plan steps ----------------------------------------------------------------------------------------------------------
// What one step of a plan (a single op, or a fused group led by its first op) launches: decided once, when the plan is created,
// from the op(s) and the plan's options (api.hip: choose_conv and the choosers below); the launcher only launches what it records.
// Each kernel family has ONE geometry function in its .hip file (op, variant -> the launch, the derived values of its kernel
// arguments, whether the shape fits): its `fits` predicate, its chooser and its args builder read that and nothing restates it.
// Every refusal that depends on the op and the step alone is the chooser's; a launcher builds the arguments, picks the instance from
// the recorded template values (each one has()-checked by the chooser) and launches `dims`.  The one exception is launch_layer
// (layers.hip), whose form depends on a run-time address.
enum class y3_fuse : uint8_t {
  none,         // one op
  into_prev,    // nothing: launched by an earlier step
  stem_pair,    // MFMA stem conv + the 3x3 stride-2 conv after it (conv_fused.hip)
  resblock,     // 64-32-64 residual block (conv_fused.hip)
  block,        // 1x1 -> 128 channels + 3x3 (+ shortcut), bottleneck tensor in LDS (conv_block.hip)
  head_decode,  // detection-head conv + YOLO decode (conv_igemm.hip, conv_1x1.hip)
  spp,          // SPP pyramid: the op and the next two, pools 5 / 9 / 13 of one tensor (layers.hip)
};
struct y3_step;
// ops: the step's op(s); d_in: the input of ops[0] (the plan input where it reads that)
typedef int (*y3_launcher)(const y3_op *ops, const y3_step &st, const void *d_in, const void *d_zero, hipStream_t s);
struct y3_step {
  y3_fuse fuse = y3_fuse::none;
  y3_launcher launch = nullptr;
  const char *name = "";
  // variant parameters (template values), each launcher reading its own: implicit GEMM version / pipeline stages / pixel x channel
  // tile; the halo kernel's pixel tile (192 / 256) and weight-ring slots (ns); the 1x1-dw and head-dw tile height (bm); the
  // weights-resident channel tile (bn); dw48 waves per workgroup; decode lanes per box; block-fused tile; pipelined (or
  // phase-by-phase) stem pair
  int version = 0, ns = 0, bm = 0, bn = 0, waves = 0, lanes = 0, tw = 0, th = 0;
  bool pipelined = false;
  y3_dims dims;                   // the launch itself (a persistent kernel's grid is an ordinary small grid)
  bool frag = false;              // reads the fragment-order copy of ops[0]'s weights (y3_conv_halo_dw_make_weights) ...
  const void *frag_w = nullptr;   // ... this one (never null at launch)
};

// choosers implemented in the .hip files: fill the step (launcher, kernel name, variant) or return an error for a shape the
// kernel family cannot take
int y3_choose_conv_igemm(const y3_op &op, const y3_options &o, y3_step &st, int force_version = 0, int force_ns = 0,
                         int force_bm = 0);   // force_*: 0 = the options' igemm_version / igemm_ns / igemm_bm
int y3_choose_conv_small(const y3_op &op, y3_step &st);
int y3_choose_conv_direct(const y3_op &op, y3_step &st);
bool y3_conv_stem_mfma_supported(const y3_op &op);
int y3_choose_conv_stem_mfma(const y3_op &op, y3_step &st);
int y3_choose_layer(const y3_op &op, y3_step &st);   // max-pool, upsample, add, copy (layers.hip)
int y3_choose_reorg(const y3_op &op, y3_step &st);   // Darknet's [reorg], both forms (layers.hip)
int y3_choose_yolo(const y3_op &op, const y3_options &o, y3_step &st);
// Fused groups: true (and the step filled) when the kernel takes the group
bool y3_choose_maxpool_spp(const y3_op &a, const y3_op &b, const y3_op &c, y3_step &st);
// first two layers of Darknet-53 as one kernel (conv_fused.hip); op1 must read only op0's output
bool y3_choose_conv_fused_stem_s2(const y3_op &op0, const y3_op &op1, const y3_options &o, y3_step &st);
bool y3_choose_conv_fused_resblock(const y3_op &op0, const y3_op &op1, const y3_options &o, y3_step &st);
bool y3_choose_conv_block_fused(const y3_op &op0, const y3_op &op1, const y3_options &o, y3_step &st);
// its direct-weights form (conv_block_dw.hip, libyolov3_hip_block.so; y3_options.fuse_block = 3 / 4): whether a pair the chooser
// above accepts carries what it needs, the step on tw x th rectangles, and whether an op can be a member of such a pair
bool y3_conv_block_dw_fits(const y3_op &op0, const y3_op &op1);
void y3_choose_conv_block_dw(const y3_op &op0, int tw, int th, y3_step &st);
bool y3_conv_block_dw_member(const y3_op &op, const y3_options &o);
// detection head: 1x1 conv + YOLO decode in one launch (conv_igemm.hip: the tiled form and the choice between the two; conv_1x1.hip:
// the direct-weights form, which reads the fragment-order copy of the head conv's weights)
bool y3_choose_conv_head_decode(const y3_op &op0, const y3_op &op1, const y3_options &o, y3_step &st);
bool y3_conv_head_dw_fits(const y3_op &op0, const y3_options &o);
void y3_choose_conv_head_decode_dw(const y3_op &op0, const y3_options &o, y3_step &st);
// halo-reuse 3x3 kernel (conv_halo.hip): whether it can take this conv, and its chooser
bool y3_conv_halo_ws_fits(const y3_op &op);
bool y3_conv_halo_dw_fits(const y3_op &op);
bool y3_conv_halo_dw_pays(const y3_op &op, const y3_options &o);
size_t y3_conv_halo_dw_weight_bytes(const y3_op &op);
int y3_conv_halo_dw_make_weights(const y3_op &op, void *dst, hipStream_t s);
int y3_choose_conv_halo_dw(const y3_op &op, y3_step &st);
int y3_choose_conv_halo(const y3_op &op, const y3_options &o, y3_step &st);
// 1x1 conv with LDS-resident weights, persistent workgroups (conv_1x1.hip)
bool y3_conv1x1_wres_supported(const y3_op &op);
bool y3_conv1x1_wres_pays(const y3_op &op);
int y3_choose_conv1x1_wres(const y3_op &op, y3_step &st);
// direct-weights 1x1 kernel for the short-K bottleneck layers on small maps (conv_1x1.hip; fragment-order weights)
bool y3_conv1x1_dw_pays(const y3_op &op);
int y3_choose_conv1x1_dw(const y3_op &op, y3_step &st);
// small-grid direct-weights kernel, 1x1 and 3x3 (conv_dw48.hip; fragment-order weights): 48-pixel x 32..256-channel tiles
bool y3_conv_dw48_fits(const y3_op &op, const y3_options &o);
bool y3_conv_dw48_fits_wide(const y3_op &op, const y3_options &o);
int y3_choose_conv_dw48(const y3_op &op, const y3_options &o, y3_step &st);
// 2-D patch form of the halo kernel for rows wider than 128 pixels (conv_halo.hip)
bool y3_conv_patch_fits(const y3_op &op);
int y3_choose_conv_patch(const y3_op &op, y3_step &st);
// true when the MFMA implicit-GEMM kernel can take this conv
bool y3_conv_igemm_supported(const y3_op &op);
// Grouped convs (y3_op.groups > 1; conv_grouped.hip).  conv_path (api.hip) asks about them before anything else, so no other
// single-op chooser ever sees one; every fused chooser declines a group that holds one.
static inline bool y3_is_grouped(const y3_op &op) { return op.kind == Y3_OP_CONV && op.groups > 1; }
// y3_set_tuning("grouped_generic", v) (api.hip): 1 sends every grouped op to conv_grouped_*
int y3_grouped_generic();
// depthwise kernel: whether the op is on its grain (then y3_conv_path answers 5 unless grouped_generic), and its chooser
bool y3_conv_dwise_fits(const y3_op &op);
int y3_choose_conv_dwise(const y3_op &op, y3_step &st);
// every other grouped op (y3_conv_path answers 4)
int y3_choose_conv_grouped(const y3_op &op, y3_step &st);
// [avgpool], [scale_channels] and [sam] (attention.hip, libyolov3_hip_attn.so)
int y3_choose_attention(const y3_op &op, y3_step &st);
