// Memory-bound NHWC layer kernels: max-pool, nearest upsample, add, channel-slice copy, reorg.
// One thread moves one 16-byte channel chunk of one output pixel when strides allow it
// (VEC = 16 / sizeof(T)), else one element (VEC = 1).  All of them take pixel strides
// (in_ld / out_ld) so producers write straight into route-concat buffers
// (/root/reference/yolov3/darknet.py:369-375) and no concat copy is needed on the usual path.
#include "common.h"
#include <initializer_list>
#include <type_traits>

namespace {

struct LayerArgs {
  const void *in;
  const void *in2;
  void *out;
  int B, H, W, C, in_ld, in2_ld, Ho, Wo, out_ld, k, stride, zero_pad, pad_lo;
  long long total;  // B*Ho*Wo*(C/VEC)
};

template <typename T, int VEC>
struct Vec {
  T v[VEC];
};

template <typename T, int VEC>
__device__ __forceinline__ void load_vec(const T *p, float out[VEC]) {
  if constexpr (VEC == 1) {
    out[0] = y3_to_float<T>(*p);
  } else {
    const u32x4 raw = *reinterpret_cast<const u32x4 *>(p);
    if constexpr (sizeof(T) == 4) {
      const f32x4 f = __builtin_bit_cast(f32x4, raw);
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = f[j];
    } else {
      float v8[8];
      y3_unpack8<T>(v8, raw);
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = v8[j];
    }
  }
}

template <typename T, int VEC>
__device__ __forceinline__ void store_vec(T *p, const float in[VEC]) {
  if constexpr (VEC == 1) {
    *p = y3_from_float<T>(in[0]);
  } else if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<f32x4 *>(p) = f32x4{in[0], in[1], in[2], in[3]};
  } else {
    float v8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v8[j] = in[j];
    *reinterpret_cast<u32x4 *>(p) = y3_pack8<T>(v8);
  }
}

__device__ __forceinline__ void decode_idx(long long idx, int cgroups, int Wo, int Ho, int &b, int &oy,
                                           int &ox, int &cg) {
  cg = (int)(idx % cgroups);
  long long pix = idx / cgroups;
  ox = (int)(pix % Wo);
  pix /= Wo;
  oy = (int)(pix % Ho);
  b = (int)(pix / Ho);
}

// ---- max-pool arithmetic: integer keys -----------------------------------------------------------------------------------
// Every max-pool here (element-wise, 16-byte wide, the SPP pyramid; both padding rules; three element types) takes its
// maximum on unsigned integer keys, not on floats.  The rule ("The layer kernels on every storage pattern"): IEEE
// 754-2019 `maximum` of the taps that count, +0 above -0, the winner's bits returned unchanged, a NaN tap left out, -inf when
// nothing is left.  With U the unsigned integer of the element's size, SIGN its top bit, INF the pattern of +inf, R = ~SIGN - INF
// (all mantissa bits) and arithmetic modulo 2^bits:
//   u = p ^ (p negative ? all ones : SIGN)    sign-magnitude -> unsigned order: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN,
//                                             -inf at R, +inf at ~R;
//   v = u + R                                 rotates the positive NaNs (u > ~R) round to [0, R), below everything; the negative
//                                             NaNs follow at [R, 2R), -inf lands on 2R, the order of the rest is kept;
//   key = max(v, 2R)                          every NaN becomes -inf, the identity of max: exactly "left out", and -inf if all are
//                                             (CLAMP = false leaves this to a running maximum that starts at 2R: the single pools).
// Unsigned max on keys is then the rule, in any order and any grouping: a cascade and a scan give the same bits.  Back:
// u = key - R, p = u ^ (u has its top bit ? SIGN : all ones).  Five packed integer instructions per tap (v_pk_ashrrev_i16, v_or,
// v_xor, v_pk_add_u16, v_pk_max_u16) and one per maximum.  No float instruction touches the data, so neither the denormal mode nor
// the quieting of a signalling NaN (v_max_f32 answers one with a quiet NaN, and a bf16 widened by a shift can be one) has a say.
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

template <typename T>
struct PoolBits;
template <>
struct PoolBits<float> {
  typedef uint32_t U;
  typedef int32_t S;
  typedef u32x4 V;
  typedef i32x4 SV;
  static constexpr U SIGN = 0x80000000u, R = 0x007FFFFFu;
};
template <>
struct PoolBits<bf16_t> {
  typedef uint16_t U;
  typedef int16_t S;
  typedef u16x8 V;
  typedef s16x8 SV;
  static constexpr U SIGN = 0x8000, R = 0x007F;
};
template <>
struct PoolBits<f16_t> {
  typedef uint16_t U;
  typedef int16_t S;
  typedef u16x8 V;
  typedef s16x8 SV;
  static constexpr U SIGN = 0x8000, R = 0x03FF;
};
// the key of -inf: what a tap left out counts as, and what an empty maximum is
template <typename T>
__device__ __forceinline__ constexpr typename PoolBits<T>::U pool_least() {
  return (typename PoolBits<T>::U)(2 * PoolBits<T>::R);
}
// the key of +0 (a padded tap of the reference's rule): u = SIGN, v = SIGN + R
template <typename T>
__device__ __forceinline__ constexpr typename PoolBits<T>::U pool_zero() {
  return (typename PoolBits<T>::U)(PoolBits<T>::SIGN + PoolBits<T>::R);
}

// one element (U) ...
__device__ __forceinline__ uint16_t pool_max(uint16_t a, uint16_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t pool_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
template <typename T, bool CLAMP = true>
__device__ __forceinline__ typename PoolBits<T>::U pool_key(typename PoolBits<T>::U p) {
  typedef PoolBits<T> P;
  typedef typename P::U U;
  const U x = (U)((U)((typename P::S)p >> (8 * sizeof(U) - 1)) | P::SIGN);
  const U v = (U)((U)(p ^ x) + P::R);
  return CLAMP ? pool_max(v, pool_least<T>()) : v;
}
template <typename T>
__device__ __forceinline__ typename PoolBits<T>::U pool_unkey(typename PoolBits<T>::U k) {
  typedef PoolBits<T> P;
  typedef typename P::U U;
  const U u = (U)(k - P::R);
  return (U)(u ^ (U)((U)~(U)((typename P::S)u >> (8 * sizeof(U) - 1)) | P::SIGN));
}
// ... and the 16 bytes of one load (V: 8 x uint16 or 4 x uint32)
__device__ __forceinline__ u16x8 pool_max(const u16x8 &a, const u16x8 &b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ u32x4 pool_max(const u32x4 &a, const u32x4 &b) { return __builtin_elementwise_max(a, b); }
template <typename T, bool CLAMP = true>
__device__ __forceinline__ typename PoolBits<T>::V pool_key(typename PoolBits<T>::V p) {
  typedef PoolBits<T> P;
  typedef typename P::V V;
  typedef typename P::U U;
  const V x = __builtin_bit_cast(V, __builtin_bit_cast(typename P::SV, p) >> (typename P::S)(8 * sizeof(U) - 1)) | P::SIGN;
  const V v = (p ^ x) + P::R;
  return CLAMP ? pool_max(v, (V)(pool_least<T>())) : v;
}
template <typename T>
__device__ __forceinline__ typename PoolBits<T>::V pool_unkey(typename PoolBits<T>::V k) {
  typedef PoolBits<T> P;
  typedef typename P::V V;
  typedef typename P::U U;
  const V u = k - P::R;
  return u ^ (~__builtin_bit_cast(V, __builtin_bit_cast(typename P::SV, u) >> (typename P::S)(8 * sizeof(U) - 1)) | P::SIGN);
}

// what one thread of a single pool holds: one element or one 16-byte chunk, as patterns
template <typename T, int VEC>
struct PoolChunk {
  typedef typename std::conditional<VEC == 1, typename PoolBits<T>::U, typename PoolBits<T>::V>::type X;
  static __device__ __forceinline__ X splat(typename PoolBits<T>::U v) {
    if constexpr (VEC == 1) return v; else return (X)(v);
  }
};

// Reference MaxPool2d.forward (darknet.py:21-29): stride 1 & k > 1 -> window [y, y+k) x [x, x+k)
// with out-of-range taps contributing 0.0 (zero padding right/bottom); otherwise floor-mode
// pooling without padding (all taps in range).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void maxpool_kernel(LayerArgs p) {
  typedef typename PoolChunk<T, VEC>::X X;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  int b, oy, ox, cg;
  decode_idx(idx, p.C / VEC, p.Wo, p.Ho, b, oy, ox, cg);
  X best = PoolChunk<T, VEC>::splat(pool_least<T>());
  bool padded = false;
  for (int ky = 0; ky < p.k; ++ky) {
    const int iy = oy * p.stride + ky;
    for (int kx = 0; kx < p.k; ++kx) {
      const int ix = ox * p.stride + kx;
      if (iy >= p.H || ix >= p.W) {
        padded = true;
        continue;
      }
      const X v = *reinterpret_cast<const X *>(static_cast<const T *>(p.in) + (((long long)b * p.H + iy) * p.W + ix) * p.in_ld + cg * VEC);
      best = pool_max(best, pool_key<T, false>(v));
    }
  }
  if (padded && p.zero_pad) best = pool_max(best, PoolChunk<T, VEC>::splat(pool_zero<T>()));   // a padded tap is a +0 tap
  *reinterpret_cast<X *>(static_cast<T *>(p.out) + (((long long)b * p.Ho + oy) * p.Wo + ox) * p.out_ld + cg * VEC) = pool_unkey<T>(best);
}

// Darknet's rule (Y3_F_POOL_DARKNET; include/yolov3_hip.h): the window of output (oy, ox) starts at
// (oy * stride - pad_lo, ox * stride - pad_lo) with pad_lo = padding / 2, and only its taps inside [0, H) x [0, W)
// count: the tap ranges are clipped up front, nothing stands in for the taps left out.  y3_choose_layer has checked that
// no window is empty, so `best` stays at its -inf start only where every tap is NaN or -inf.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void maxpool_dk_kernel(LayerArgs p) {
  typedef typename PoolChunk<T, VEC>::X X;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  int b, oy, ox, cg;
  decode_idx(idx, p.C / VEC, p.Wo, p.Ho, b, oy, ox, cg);
  const int y0 = oy * p.stride - p.pad_lo, x0 = ox * p.stride - p.pad_lo;
  const int ky0 = y0 < 0 ? -y0 : 0, ky1 = min(p.k, p.H - y0);
  const int kx0 = x0 < 0 ? -x0 : 0, kx1 = min(p.k, p.W - x0);
  X best = PoolChunk<T, VEC>::splat(pool_least<T>());
  for (int ky = ky0; ky < ky1; ++ky) {
    const T *row = static_cast<const T *>(p.in) + (((long long)b * p.H + y0 + ky) * p.W + x0) * p.in_ld + cg * VEC;
    for (int kx = kx0; kx < kx1; ++kx)
      best = pool_max(best, pool_key<T, false>(*reinterpret_cast<const X *>(row + (long long)kx * p.in_ld)));
  }
  *reinterpret_cast<X *>(static_cast<T *>(p.out) + (((long long)b * p.Ho + oy) * p.Wo + ox) * p.out_ld + cg * VEC) = pool_unkey<T>(best);
}

// nn.Upsample(scale_factor, mode="nearest") (darknet.py:302-305)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void upsample_kernel(LayerArgs p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  int b, oy, ox, cg;
  decode_idx(idx, p.C / VEC, p.Wo, p.Ho, b, oy, ox, cg);
  const int iy = oy / p.stride, ix = ox / p.stride;
  float v[VEC];
  load_vec<T, VEC>(static_cast<const T *>(p.in) + (((long long)b * p.H + iy) * p.W + ix) * p.in_ld + cg * VEC, v);
  store_vec<T, VEC>(static_cast<T *>(p.out) + (((long long)b * p.Ho + oy) * p.Wo + ox) * p.out_ld + cg * VEC, v);
}

// shortcut that could not be fused into a conv epilogue (darknet.py:379)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void add_kernel(LayerArgs p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  int b, oy, ox, cg;
  decode_idx(idx, p.C / VEC, p.Wo, p.Ho, b, oy, ox, cg);
  const long long pix = ((long long)b * p.Ho + oy) * p.Wo + ox;
  float x[VEC], y[VEC];
  load_vec<T, VEC>(static_cast<const T *>(p.in) + pix * p.in_ld + cg * VEC, x);
  load_vec<T, VEC>(static_cast<const T *>(p.in2) + pix * p.in2_ld + cg * VEC, y);
#pragma unroll
  for (int j = 0; j < VEC; ++j) x[j] += y[j];
  store_vec<T, VEC>(static_cast<T *>(p.out) + pix * p.out_ld + cg * VEC, x);
}

// route member that could not be produced in place (darknet.py:372-375)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void copy_kernel(LayerArgs p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  int b, oy, ox, cg;
  decode_idx(idx, p.C / VEC, p.Wo, p.Ho, b, oy, ox, cg);
  const long long pix = ((long long)b * p.Ho + oy) * p.Wo + ox;
  float x[VEC];
  load_vec<T, VEC>(static_cast<const T *>(p.in) + pix * p.in_ld + cg * VEC, x);
  store_vec<T, VEC>(static_cast<T *>(p.out) + pix * p.out_ld + cg * VEC, x);
}

enum Which { MAXPOOL, MAXPOOL_DK, UPSAMPLE, ADD, COPY };

template <typename T, int VEC>
void launch_one(Which w, const LayerArgs &a, hipStream_t s) {
  const dim3 grid((unsigned)((a.total + 255) / 256)), block(256);
  switch (w) {
    case MAXPOOL: Y3_LAUNCH((maxpool_kernel<T, VEC>), grid, block, 0, s, a); break;
    case MAXPOOL_DK: Y3_LAUNCH((maxpool_dk_kernel<T, VEC>), grid, block, 0, s, a); break;
    case UPSAMPLE: Y3_LAUNCH((upsample_kernel<T, VEC>), grid, block, 0, s, a); break;
    case ADD: Y3_LAUNCH((add_kernel<T, VEC>), grid, block, 0, s, a); break;
    case COPY: Y3_LAUNCH((copy_kernel<T, VEC>), grid, block, 0, s, a); break;
  }
}

// the wide form (one 16-byte channel chunk per thread) or the element-wise one: decided at launch, from the op and its input
bool layer_is_wide(const y3_op &op, const void *d_in) {
  const int vec = 16 / y3_elem_size(op.dtype);
  bool wide = op.in_c % vec == 0 && op.in_ld % vec == 0 && op.out_ld % vec == 0 &&
              ((uintptr_t)d_in % 16 == 0) && ((uintptr_t)op.d_out % 16 == 0);
  if (op.kind == Y3_OP_ADD) wide = wide && op.res_ld % vec == 0 && ((uintptr_t)op.d_res % 16 == 0);
  return wide;
}
long long layer_threads(const y3_op &op, bool wide) {
  return (long long)op.batch * op.out_h * op.out_w * (wide ? op.in_c / (16 / y3_elem_size(op.dtype)) : op.in_c);
}

int launch_layer(const y3_op *ops, const y3_step &, const void *d_in, const void *, hipStream_t s) {
  const y3_op &op = ops[0];
  const Which w = op.kind == Y3_OP_MAXPOOL ? ((op.flags & Y3_F_POOL_DARKNET) ? MAXPOOL_DK : MAXPOOL) : op.kind == Y3_OP_UPSAMPLE ? UPSAMPLE : op.kind == Y3_OP_ADD ? ADD : COPY;
  LayerArgs a;
  a.in = d_in;
  a.in2 = op.d_res;
  a.out = op.d_out;
  a.B = op.batch; a.H = op.in_h; a.W = op.in_w; a.C = op.in_c; a.in_ld = op.in_ld; a.in2_ld = op.res_ld;
  a.Ho = op.out_h; a.Wo = op.out_w; a.out_ld = op.out_ld;
  a.k = op.ksize; a.stride = op.stride;
  a.zero_pad = (op.ksize > 1 && op.stride == 1) ? 1 : 0;
  a.pad_lo = op.pad / 2;
  const bool wide = layer_is_wide(op, d_in);
  a.total = layer_threads(op, wide);
  Y3_REQUIRE(a.total <= kY3MaxThreads, "block %d: a launch of %lld threads; the limit is %lld", op.block_idx, a.total, kY3MaxThreads);
  return y3_by_dtype(op.dtype, [&](auto tag) {
    typedef decltype(tag) T;
    if (wide) launch_one<T, 16 / sizeof(T)>(w, a, s); else launch_one<T, 1>(w, a, s);
    Y3_HIP_CHECK(hipGetLastError());
    return Y3_OK;
  });
}

}  // namespace

int y3_choose_layer(const y3_op &op, y3_step &st) {
  Y3_REQUIRE(op.in_c == op.out_c, "block %d: channel count changes in a pool/upsample/add/copy op", op.block_idx);
  // one thread per 16-byte chunk or per element of the output (an op that reads the plan's input: its address is not known yet
  // and is taken as aligned; launch_layer checks what it really launches)
  st.dims = {y3_ceil_div64(layer_threads(op, layer_is_wide(op, (op.flags & Y3_F_PLAN_INPUT) ? nullptr : op.d_in)), 256), 256, 0};
  st.launch = launch_layer;
  switch (op.kind) {
    case Y3_OP_MAXPOOL:
      Y3_REQUIRE(op.ksize >= 1 && op.stride >= 1, "maxpool block %d: bad size/stride", op.block_idx);
      if (op.flags & Y3_F_POOL_DARKNET) {
        Y3_REQUIRE(op.pad >= 0, "maxpool block %d: negative padding %d", op.block_idx, op.pad);
        Y3_REQUIRE(op.in_h + op.pad >= op.ksize && op.in_w + op.pad >= op.ksize,
                   "maxpool block %d: size %d does not fit the padded %d x %d map (padding %d)", op.block_idx, op.ksize, op.in_h, op.in_w, op.pad);
        Y3_REQUIRE(op.out_h == (op.in_h + op.pad - op.ksize) / op.stride + 1 && op.out_w == (op.in_w + op.pad - op.ksize) / op.stride + 1,
                   "maxpool block %d: output size mismatch (Darknet rule: (in + padding - size) / stride + 1)", op.block_idx);
        // first window ends at size - 1 - padding / 2, last window starts at (out - 1) * stride - padding / 2: both must
        // touch the image, or an output would be the max of nothing
        Y3_REQUIRE(op.pad / 2 < op.ksize && (op.out_h - 1) * op.stride - op.pad / 2 < op.in_h && (op.out_w - 1) * op.stride - op.pad / 2 < op.in_w,
                   "maxpool block %d: padding %d leaves a window of size %d without a tap inside the %d x %d map", op.block_idx, op.pad,
                   op.ksize, op.in_h, op.in_w);
        st.name = Y3_KNAME(op.dtype, "maxpool_dk_", "");
        return Y3_OK;
      }
      if (op.stride == 1) {
        Y3_REQUIRE(op.out_h == op.in_h && op.out_w == op.in_w, "maxpool block %d: stride-1 keeps H,W", op.block_idx);
      } else {
        Y3_REQUIRE(op.out_h == (op.in_h - op.ksize) / op.stride + 1 && op.out_w == (op.in_w - op.ksize) / op.stride + 1,
                   "maxpool block %d: output size mismatch", op.block_idx);
      }
      st.name = Y3_KNAME(op.dtype, "maxpool_", "");
      return Y3_OK;
    case Y3_OP_UPSAMPLE:
      Y3_REQUIRE(op.stride >= 1 && op.out_h == op.in_h * op.stride && op.out_w == op.in_w * op.stride,
                 "upsample block %d: output size mismatch", op.block_idx);
      st.name = Y3_KNAME(op.dtype, "upsample_", "");
      return Y3_OK;
    case Y3_OP_ADD:
      Y3_REQUIRE(op.out_h == op.in_h && op.out_w == op.in_w, "add block %d: size mismatch", op.block_idx);
      st.name = Y3_KNAME(op.dtype, "add_", "");
      return Y3_OK;
    default:
      Y3_REQUIRE(op.out_h == op.in_h && op.out_w == op.in_w, "copy block %d: size mismatch", op.block_idx);
      st.name = Y3_KNAME(op.dtype, "copy_", "");
      return Y3_OK;
  }
}

// ------------------------------------------------------------------------------------------------
// Darknet's [reorg] (Y3_OP_REORG; include/yolov3_hip.h), YOLOv2's pass-through layer: (C, H, W) per frame ->
// (C*s*s, H/s, W/s), a pure move of storage elements (U = an unsigned integer of the element's size, so every dtype is
// bit-exact).  Both forms are defined on the frame's NCHW arrays; the tensors here are NHWC with pixel strides, so one thread
// takes one OUTPUT element (adjacent threads: adjacent output channels, i.e. coalesced stores into the route's channel
// slice), works out the NCHW coordinates of its source and gathers it:
//   flat form  : the output element (ko, oy, ox) is number f = ox + Wo*(oy + Ho*ko) of the frame's flat array; Darknet
//                writes out_flat[f] = in_flat[src] with f read as (k, j, i) of the INPUT shape, c2 = k % oc, off = k / oc,
//                src = (i*s + off % s) + (W*s)*((j*s + off / s) + (H*s)*c2), and src is read as (ci, yi, xi) of the input shape;
//   3d form    : g = ko / C, source (ko % C, oy*s + g / s, ox*s + g % s).
// y3_choose_reorg has checked the divisibility the formulas rely on, so src < C*H*W (flat) and yi < H, xi < W (3d).
// The yolov2 layer is 64 x 26 x 26 per frame, about 1 % of the network's traffic: no LDS staging, no tuning.
namespace {

struct ReorgArgs {
  const void *in;
  void *out;
  int C, H, W, in_ld, Co, Ho, Wo, out_ld, s, oc, form3d;
  long long total;  // B*Ho*Wo*Co
};

template <typename U>
__global__ __launch_bounds__(256) void reorg_kernel(ReorgArgs p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  int b, oy, ox, ko;
  decode_idx(idx, p.Co, p.Wo, p.Ho, b, oy, ox, ko);
  int ci, yi, xi;
  if (p.form3d) {
    const int g = ko / p.C;
    ci = ko - g * p.C;
    yi = oy * p.s + g / p.s;
    xi = ox * p.s + g % p.s;
  } else {
    const int f = ox + p.Wo * (oy + p.Ho * ko);
    const int i = f % p.W, jk = f / p.W, j = jk % p.H, k = jk / p.H;
    const int c2 = k % p.oc, off = k / p.oc;
    const int src = (i * p.s + off % p.s) + (p.W * p.s) * ((j * p.s + off / p.s) + (p.H * p.s) * c2);
    xi = src % p.W;
    const int yc = src / p.W;
    yi = yc % p.H;
    ci = yc / p.H;
  }
  static_cast<U *>(p.out)[(((long long)b * p.Ho + oy) * p.Wo + ox) * p.out_ld + ko] =
      static_cast<const U *>(p.in)[(((long long)b * p.H + yi) * p.W + xi) * p.in_ld + ci];
}

int launch_reorg(const y3_op *ops, const y3_step &st, const void *d_in, const void *, hipStream_t s) {
  const y3_op &op = ops[0];
  ReorgArgs a;
  a.in = d_in;
  a.out = op.d_out;
  a.C = op.in_c; a.H = op.in_h; a.W = op.in_w; a.in_ld = op.in_ld;
  a.Co = op.out_c; a.Ho = op.out_h; a.Wo = op.out_w; a.out_ld = op.out_ld;
  a.s = op.stride;
  a.oc = op.in_c / (op.stride * op.stride);
  a.form3d = (op.flags & Y3_F_REORG_3D) ? 1 : 0;
  a.total = (long long)op.batch * op.out_h * op.out_w * op.out_c;
  return y3_elem_size(op.dtype) == 4 ? y3_launch<reorg_kernel<uint32_t>>(st.dims, s, a) : y3_launch<reorg_kernel<uint16_t>>(st.dims, s, a);
}

}  // namespace

int y3_choose_reorg(const y3_op &op, y3_step &st) {
  const int s = op.stride;
  Y3_REQUIRE(!(op.flags & (Y3_F_PLAN_INPUT | Y3_F_IN_NCHW_F32 | Y3_F_IN_NHWC_U8BGR | Y3_F_OUT_F32)),
             "reorg block %d: reads and writes NHWC tensors of the plan's element type only", op.block_idx);
  Y3_REQUIRE(s >= 1 && s <= 64, "reorg block %d: stride %d (1..64)", op.block_idx, s);
  Y3_REQUIRE(op.in_h % s == 0 && op.in_w % s == 0, "reorg block %d: stride %d does not divide the %d x %d map", op.block_idx, s,
             op.in_h, op.in_w);
  Y3_REQUIRE((op.flags & Y3_F_REORG_3D) || op.in_c % (s * s) == 0,
             "reorg block %d: %d channels are not a multiple of stride^2 = %d (the flat form needs it)", op.block_idx, op.in_c, s * s);
  Y3_REQUIRE(op.out_h == op.in_h / s && op.out_w == op.in_w / s && (long long)op.out_c == (long long)op.in_c * s * s,
             "reorg block %d: output shape mismatch (C*s*s, H/s, W/s)", op.block_idx);
  Y3_REQUIRE(op.in_ld >= op.in_c && op.out_ld >= op.out_c, "reorg block %d: pixel stride below the channel count (in %d < %d or out %d < %d)",
             op.block_idx, op.in_ld, op.in_c, op.out_ld, op.out_c);
  // (the kernel keeps a frame's flat NCHW indices in int)
  Y3_REQUIRE((long long)op.in_c * op.in_h * op.in_w < (1ll << 31), "reorg block %d: a frame of %d x %d x %d elements is too large",
             op.block_idx, op.in_c, op.in_h, op.in_w);
  st.launch = launch_reorg;
  st.dims = {y3_ceil_div64((long long)op.batch * op.out_h * op.out_w * op.out_c, 256), 256, 0};   // one thread per output element
  st.name = (op.flags & Y3_F_REORG_3D) ? Y3_KNAME(op.dtype, "reorg3d_", "") : Y3_KNAME(op.dtype, "reorg_", "");
  return Y3_OK;
}

// ------------------------------------------------------------------------------------------------
// SPP pyramid (models/yolov3-spp.cfg:576-595): three stride-1 "same" max-pools of sizes 5 / 9 / 13 that read ONE
// tensor and feed one route concat, as ONE launch.  Reference semantics (darknet.py:16-29): window
// [y, y+k) x [x, x+k), out-of-range taps contribute 0.0 (ZeroPad2d right/bottom, then an unpadded pool).
//
// One workgroup = one frame x one 32-byte channel group (16 bf16 / 8 float32 channels).  The (H+12) x (W+12)
// zero-padded image of that group is staged in LDS once (16-byte vectors, two per position; as integer keys, NaN taps as
// -inf: "max-pool arithmetic" above), then the pyramid is a cascade, exact because max is associative and the windows nest:
//   R5[y][x]  = max(A[y][x .. x+4])                               (row pass)
//   P5[y][x]  = max(R5[y .. y+4][x])                              on (H+8) x (W+8)
//   P9[y][x]  = max(P5[y][x], P5[y+4][x], P5[y][x+4], P5[y+4][x+4])   on (H+4) x (W+4)   ([y,y+9) = [y,y+5) u [y+4,y+9))
//   P13[y][x] = max of the same four taps of P9                   on H x W
// 4 + 4 + 3 + 3 = 14 LDS reads per output vector instead of 25 + 81 + 169 global loads, and each result goes
// straight into its channel slice of the concat buffer (out pointers / pixel stride of the three ops).
//
// Darknet's rule (DK = true; Y3_F_POOL_DARKNET with padding = k - 1 on all three ops): window [y - k/2, y + k/2] x
// [x - k/2, x + k/2], out-of-range taps ignored.  The cascade above only ever combines tile positions, so it does not care
// where the image sits in the tile: stage the image at offset (6, 6) of the same (H+12) x (W+12) tile and fill the border
// with -inf of the element type (the identity of max, so a border tap is a tap left out).  Tile position t = image
// position t - 6, and Pk[ty][tx] covers tile rows [ty, ty+k), i.e. image rows [ty - 6, ty - 6 + k):
//   13 x 13 at (y, x): image rows [y-6, y+6] = tile rows [y,   y+12]  -> P13[y][x]
//    9 x  9 at (y, x): image rows [y-4, y+4] = tile rows [y+2, y+10]  -> P9[y+2][x+2]     (y+2 <= H+1, inside P9's H+4 rows)
//    5 x  5 at (y, x): image rows [y-2, y+2] = tile rows [y+4, y+8]   -> P5[y+4][x+4]     (y+4 <= H+3, inside P5's H+8 rows)
// so the same five steps run, with the stores of steps 3 / 4 taken from tile rows and columns [4, H+4) / [2, H+2) instead
// of [0, H).  Every window holds its own centre, so no result is -inf unless the image is.  Same LDS, same reads, same grid.
namespace {

struct SppArgs {
  const char *in;
  char *out5, *out9, *out13;
  int H, W, in_ld, ld5, ld9, ld13, cgroups;
};

// the tile holds keys (pool_key above): staged once, combined with integer max, turned back into patterns at the stores
template <typename T>
__device__ __forceinline__ u32x4 vmax16(const u32x4 &a, const u32x4 &b) {
  typedef typename PoolBits<T>::V V;
  return __builtin_bit_cast(u32x4, pool_max(__builtin_bit_cast(V, a), __builtin_bit_cast(V, b)));
}
template <typename T>
__device__ __forceinline__ u32x4 spp_key(const u32x4 &raw) {
  return __builtin_bit_cast(u32x4, pool_key<T>(__builtin_bit_cast(typename PoolBits<T>::V, raw)));
}
template <typename T>
__device__ __forceinline__ u32x4 spp_unkey(const u32x4 &k) {
  return __builtin_bit_cast(u32x4, pool_unkey<T>(__builtin_bit_cast(typename PoolBits<T>::V, k)));
}

template <typename T, bool DK>
__global__ __launch_bounds__(256) void maxpool_spp_kernel(SppArgs p) {
  extern __shared__ __attribute__((aligned(16))) u32x4 spp_lds[];
  constexpr int ES = sizeof(T), V = 2;                 // 16-byte vectors per position
  const int PH = p.H + 12, PW = p.W + 12;
  const int b = blockIdx.x / p.cgroups, cg = blockIdx.x - b * p.cgroups;
  u32x4 *A = spp_lds, *Bf = spp_lds + PH * PW * V;
  const int tid = threadIdx.x;
  const long long frame = (long long)b * p.H * p.W;
  // image origin in the tile; tile origin of the 5 x 5 / 9 x 9 results (the 13 x 13 ones start at 0 either way)
  constexpr int O = DK ? 6 : 0, S5 = DK ? 4 : 0, S9 = DK ? 2 : 0;
  // border value, as a key: +0, or -inf of the element type
  constexpr uint32_t EDGE = DK ? pool_least<T>() : pool_zero<T>();
  constexpr uint32_t FILL = ES == 4 ? EDGE : (EDGE << 16 | EDGE);
  const u32x4 border = u32x4{FILL, FILL, FILL, FILL};
  // 1. stage the padded image
  for (int idx = tid; idx < PH * PW * V; idx += 256) {
    const int pos = idx >> 1, v = idx & 1, ty = pos / PW, tx = pos - ty * PW, y = ty - O, x = tx - O;
    A[idx] = ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W)
                 ? spp_key<T>(*reinterpret_cast<const u32x4 *>(p.in + ((frame + y * p.W + x) * p.in_ld) * ES + cg * 32 + v * 16))
                 : border;
  }
  __syncthreads();
  // 2. row pass of the 5 x 5 pool
  const int W5 = PW - 4, H5 = PH - 4;
  for (int idx = tid; idx < PH * W5 * V; idx += 256) {
    const int pos = idx >> 1, v = idx & 1, y = pos / W5, x = pos - y * W5;
    const u32x4 *a = A + (y * PW + x) * V + v;
    u32x4 m = vmax16<T>(a[0], a[V]);
    m = vmax16<T>(m, a[2 * V]);
    m = vmax16<T>(m, a[3 * V]);
    Bf[(y * PW + x) * V + v] = vmax16<T>(m, a[4 * V]);
  }
  __syncthreads();
  // 3. column pass -> P5 on (H+8) x (W+8), kept in A; its H x W part from (S5, S5) on is the 5 x 5 pool's output
  for (int idx = tid; idx < H5 * W5 * V; idx += 256) {
    const int pos = idx >> 1, v = idx & 1, y = pos / W5, x = pos - y * W5;
    const u32x4 *r = Bf + (y * PW + x) * V + v;
    u32x4 m = vmax16<T>(r[0], r[PW * V]);
    m = vmax16<T>(m, r[2 * PW * V]);
    m = vmax16<T>(m, r[3 * PW * V]);
    m = vmax16<T>(m, r[4 * PW * V]);
    A[(y * PW + x) * V + v] = m;
    if ((unsigned)(y - S5) < (unsigned)p.H && (unsigned)(x - S5) < (unsigned)p.W)
      *reinterpret_cast<u32x4 *>(p.out5 + ((frame + (y - S5) * p.W + (x - S5)) * p.ld5) * ES + cg * 32 + v * 16) = spp_unkey<T>(m);
  }
  __syncthreads();
  // 4. P9 on (H+4) x (W+4) from four taps of P5, kept in Bf; the 9 x 9 pool's output from (S9, S9) on
  const int W9 = PW - 8, H9 = PH - 8;
  for (int idx = tid; idx < H9 * W9 * V; idx += 256) {
    const int pos = idx >> 1, v = idx & 1, y = pos / W9, x = pos - y * W9;
    const u32x4 *a = A + (y * PW + x) * V + v;
    const u32x4 m = vmax16<T>(vmax16<T>(a[0], a[4 * V]), vmax16<T>(a[4 * PW * V], a[(4 * PW + 4) * V]));
    Bf[(y * PW + x) * V + v] = m;
    if ((unsigned)(y - S9) < (unsigned)p.H && (unsigned)(x - S9) < (unsigned)p.W)
      *reinterpret_cast<u32x4 *>(p.out9 + ((frame + (y - S9) * p.W + (x - S9)) * p.ld9) * ES + cg * 32 + v * 16) = spp_unkey<T>(m);
  }
  __syncthreads();
  // 5. P13 on H x W from four taps of P9
  for (int idx = tid; idx < p.H * p.W * V; idx += 256) {
    const int pos = idx >> 1, v = idx & 1, y = pos / p.W, x = pos - y * p.W;
    const u32x4 *a = Bf + (y * PW + x) * V + v;
    const u32x4 m = vmax16<T>(vmax16<T>(a[0], a[4 * V]), vmax16<T>(a[4 * PW * V], a[(4 * PW + 4) * V]));
    *reinterpret_cast<u32x4 *>(p.out13 + ((frame + y * p.W + x) * p.ld13) * ES + cg * 32 + v * 16) = spp_unkey<T>(m);
  }
}

size_t spp_lds_bytes(const y3_op &op) { return (size_t)(op.in_h + 12) * (op.in_w + 12) * 2 * 16 * 2; }

}  // namespace

static int launch_maxpool_spp(const y3_op *ops, const y3_step &, const void *, const void *, hipStream_t s);

// three consecutive max-pool ops of a plan.  True when they form the SPP pyramid this kernel computes: sizes {5, 9, 13} in
// any order, stride 1, the same input view, 32-byte channel groups, the image fits LDS, and one pooling rule for all three:
// none with Y3_F_POOL_DARKNET, or all with it and padding = size - 1 (the centred pool the kernel's DK form computes).  Anything
// else, a triple of mixed rules included, runs as three single pools.
bool y3_choose_maxpool_spp(const y3_op &a, const y3_op &b, const y3_op &c, y3_step &st) {
  const y3_op *o[3] = {&a, &b, &c};
  int seen = 0;
  for (const y3_op *q : o) {
    if (q->kind != Y3_OP_MAXPOOL || q->stride != 1) return false;
    if ((q->flags & Y3_F_POOL_DARKNET) != (a.flags & Y3_F_POOL_DARKNET)) return false;
    if ((q->flags & Y3_F_POOL_DARKNET) && q->pad != q->ksize - 1) return false;
    if (q->ksize == 5) seen |= 1; else if (q->ksize == 9) seen |= 2; else if (q->ksize == 13) seen |= 4; else return false;
    if (q->d_in != a.d_in || q->in_ld != a.in_ld || q->in_h != a.in_h || q->in_w != a.in_w || q->in_c != a.in_c ||
        q->batch != a.batch || q->dtype != a.dtype || (q->flags & Y3_F_PLAN_INPUT))
      return false;
    const int es = y3_elem_size(q->dtype), vec = 16 / es;
    if (q->in_c % (2 * vec) || q->in_ld % vec || q->out_ld % vec || ((uintptr_t)q->d_in % 16) || ((uintptr_t)q->d_out % 16))
      return false;
    if (q->out_h != q->in_h || q->out_w != q->in_w || q->out_c != q->in_c) return false;
  }
  if (seen != 7 || spp_lds_bytes(a) > 64 * 1024) return false;
  // one workgroup of 256 threads per frame and 32-byte channel group; past the launch limit: three single pools
  const long long grid = (long long)a.batch * (a.in_c * y3_elem_size(a.dtype) / 32);
  if (grid * 256 > kY3MaxThreads) return false;
  st.dims = {grid, 256, spp_lds_bytes(a)};
  st.launch = launch_maxpool_spp;
  st.name = (a.flags & Y3_F_POOL_DARKNET) ? Y3_KNAME(a.dtype, "maxpool_spp_pyramid_dk_", "") : Y3_KNAME(a.dtype, "maxpool_spp_pyramid_", "");
  return true;
}

static int launch_maxpool_spp(const y3_op *ops, const y3_step &st, const void *, const void *, hipStream_t s) {
  const y3_op &a = ops[0];
  const y3_op *o[3] = {&ops[0], &ops[1], &ops[2]};
  SppArgs p;
  p.in = static_cast<const char *>(a.d_in);
  p.H = a.in_h; p.W = a.in_w; p.in_ld = a.in_ld;
  p.cgroups = a.in_c * y3_elem_size(a.dtype) / 32;
  for (const y3_op *q : o) {
    if (q->ksize == 5) { p.out5 = static_cast<char *>(q->d_out); p.ld5 = q->out_ld; }
    else if (q->ksize == 9) { p.out9 = static_cast<char *>(q->d_out); p.ld9 = q->out_ld; }
    else { p.out13 = static_cast<char *>(q->d_out); p.ld13 = q->out_ld; }
  }
  return y3_by_dtype(a.dtype, [&](auto tag) {
    if (a.flags & Y3_F_POOL_DARKNET) return y3_launch<maxpool_spp_kernel<decltype(tag), true>>(st.dims, s, p);
    return y3_launch<maxpool_spp_kernel<decltype(tag), false>>(st.dims, s, p);
  });
}

// ------------------------------------------------------------------------------------------------
// Frame resize on device: uint8 HxWx3 -> net_h x net_w x 3, OpenCV's 8-bit INTER_LINEAR
// arithmetic.  Replaces the host `cv2.resize(image, (net_h, net_w))` of /root/reference/yolov3/inference.py:320-326
// for frames that are not net-sized.  Integer arithmetic only, identical to yolov3/preprocess.py:
// resize_bilinear_u8 (the tap tables -- lo index, hi index, 11-bit weights per output row / column, OpenCV's
// xofs / ialpha / yofs / ibeta -- are computed once on the host and passed in: host and device are bit-identical).
namespace {
__global__ __launch_bounds__(256) void resize_u8_kernel(const uint8_t *src, int sh, int sw, uint8_t *dst, int dh,
                                                        int dw, const int *ytab, const int *xtab) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= dh * dw) return;
  const int y = idx / dw, x = idx - y * dw;
  const int ylo = ytab[y * 4 + 0], yhi = ytab[y * 4 + 1], wy0 = ytab[y * 4 + 2], wy1 = ytab[y * 4 + 3];
  const int xlo = xtab[x * 4 + 0], xhi = xtab[x * 4 + 1], wx0 = xtab[x * 4 + 2], wx1 = xtab[x * 4 + 3];
  const uint8_t *r0 = src + (long long)ylo * sw * 3, *r1 = src + (long long)yhi * sw * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // OpenCV's two truncating stages (resize.cpp: HResizeLinear to int, then VResizeLinear<uchar, int, short, ...>)
    const int top = r0[xlo * 3 + c] * wx0 + r0[xhi * 3 + c] * wx1;
    const int bot = r1[xlo * 3 + c] * wx0 + r1[xhi * 3 + c] * wx1;
    int v = (((wy0 * (top >> 4)) >> 16) + ((wy1 * (bot >> 4)) >> 16) + 2) >> 2;
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    dst[(long long)idx * 3 + c] = (uint8_t)v;
  }
}

// Plain byte mover for buffers that a copy engine would otherwise carry: `blocks` workgroups stride over the buffer with
// 16-byte accesses, four in flight per thread.  Either side may be pinned host memory (the GPU addresses it directly).
__global__ __launch_bounds__(256) void copy_bytes_kernel(const char *__restrict__ src, char *__restrict__ dst, size_t n16, size_t tail0,
                                                          size_t nbytes) {
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const u32x4 *s4 = reinterpret_cast<const u32x4 *>(src);
  u32x4 *d4 = reinterpret_cast<u32x4 *>(dst);
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const u32x4 a = s4[i], b = s4[i + stride], c = s4[i + 2 * stride], d = s4[i + 3 * stride];
    d4[i] = a; d4[i + stride] = b; d4[i + 2 * stride] = c; d4[i + 3 * stride] = d;
  }
  for (; i < n16; i += stride) d4[i] = s4[i];
  if (blockIdx.x == 0) for (size_t t = tail0 + threadIdx.x; t < nbytes; t += 256) dst[t] = src[t];
}
}  // namespace

extern "C" int y3_copy_bytes(const void *src, void *dst, size_t nbytes, int blocks, void *stream) {
  Y3_REQUIRE(src && dst, "y3_copy_bytes: null pointer argument");
  Y3_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "y3_copy_bytes: buffers must be 16-byte aligned");
  if (nbytes == 0) return Y3_OK;
  // a pageable host pointer would be a GPU memory fault inside the kernel, not an error code: both ends must be device
  // memory or pinned / registered host memory (what the runtime knows an address for)
  for (const void *ptr : {src, static_cast<const void *>(dst)}) {
    hipPointerAttribute_t attr;
    const hipError_t e = hipPointerGetAttributes(&attr, ptr);
    if (e != hipSuccess || attr.type == hipMemoryTypeUnregistered) {
      (void)hipGetLastError();
      y3_set_error("y3_copy_bytes: %p is neither device memory nor pinned (registered) host memory", ptr);
      return Y3_ERR_INVALID;
    }
  }
  if (blocks < 1) blocks = 32;
  if (blocks > 1024) blocks = 1024;
  Y3_LAUNCH(copy_bytes_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const char *>(src), static_cast<char *>(dst), nbytes / 16, nbytes / 16 * 16, nbytes);
  Y3_HIP_CHECK(hipGetLastError());
  return Y3_OK;
}

extern "C" int y3_resize_bilinear_u8(const uint8_t *d_src, int src_h, int src_w, uint8_t *d_dst, int dst_h, int dst_w,
                                     const int32_t *d_ytab, const int32_t *d_xtab, void *stream) {
  Y3_REQUIRE(d_src && d_dst && d_ytab && d_xtab, "y3_resize_bilinear_u8: null pointer argument");
  Y3_REQUIRE(src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0, "y3_resize_bilinear_u8: empty image");
  Y3_LAUNCH(resize_u8_kernel, dim3((dst_h * dst_w + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                     d_src, src_h, src_w, d_dst, dst_h, dst_w, d_ytab, d_xtab);
  Y3_HIP_CHECK(hipGetLastError());
  return Y3_OK;
}
