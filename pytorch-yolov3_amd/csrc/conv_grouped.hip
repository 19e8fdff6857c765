// Grouped convolutions (y3_op.groups > 1): Darknet's `groups=` on a [convolutional] block.
//
//  * conv_dwise: depthwise (groups == Cin == Cout) on the 8-channel grain.  K is ksize^2 per output, so there is nothing for
//    the matrix pipes; 2 * ksize^2 FLOP per element read and written makes it memory-bound.  Built as an element-wise kernel:
//    a lane owns one 8-channel chunk (one 16-byte load / store in the 16-bit types, two in float32) of a run of kDwRun
//    output pixels along x, so that an input column it has loaded serves up to ksize outputs.  Consecutive lanes take
//    consecutive chunks, then consecutive runs: a wave's loads are contiguous wherever the tensor is.  For 3x3 the lane's
//    72 weights sit in registers as float (stride 1 and stride 2 instances); other sizes read them per tap.
//  * conv_grouped: every other grouped op (and every grouped op under y3_set_tuning("grouped_generic", 1)).  One thread per
//    pixel and 8 consecutive output channels where a group's output channels come in eights, else one thread per output
//    element as conv_direct.  A correctness path at VALU speed.
//
// Both sum a value in float32 from 0 in the order ky outermost, kx next, channel of the group innermost, every product
// rounded before it is added (this file is compiled with -ffp-contract=off), and taps outside the image add nothing: a
// depthwise op gives the same bits on either.  Both end in the shared epilogue (common.h: acc * scale + bias, activation,
// then the shortcut operand added in float32 and one rounding to the storage type).
//
// This file is a shared library of its own (libyolov3_hip_grouped.so: csrc/Makefile), a dependency of libyolov3_hip.so, whose
// device code stays byte for byte what it was; y3_set_error and the launch hooks come from the main library.
#include "common.h"

namespace {

constexpr int kDwRun = 4;   // output pixels along x per lane of conv_dwise

struct GroupedArgs {
  const void *in;
  const void *wgt;
  const float *scale;
  const float *bias;
  const void *res;
  void *out;
  int B, H, W, Cin, in_ld, Ho, Wo, Cout, out_ld, res_ld, ks, stride, pad, k_ld, groups;
  int nchunk, nxr;     // conv_dwise: 8-channel chunks per pixel, runs per output row
  int vec_in, vec_out; // conv_grouped, 8-channel form: 16-byte loads of input and weights / of the shortcut operand and stores
  long long total;     // threads that have work
  uint32_t flags;
};

// eight consecutive stored elements <-> eight floats (16 bytes in the 16-bit types, 2 x 16 in float32; p is 16-byte aligned)
template <typename T>
__device__ __forceinline__ void ld8(const T *p, float (&v)[8]) {
  if constexpr (sizeof(T) == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4 *>(p), b = *reinterpret_cast<const f32x4 *>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
  } else {
    y3_unpack8<T>(v, *reinterpret_cast<const u32x4 *>(p));
  }
}
template <typename T>
__device__ __forceinline__ void st8(T *p, const float (&v)[8]) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<f32x4 *>(p) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4 *>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
  } else {
    *reinterpret_cast<u32x4 *>(p) = y3_pack8<T>(v);
  }
}

// acc[0..7] of output pixel m, channels c0 .. c0 + 7 -> scale, bias, activation, (+ shortcut), one 8-channel store
template <typename T>
__device__ __forceinline__ void epilogue8(const GroupedArgs &p, const float (&acc)[8], long long m, int c0, int act, bool vec) {
  const f32x4 sc_lo = *reinterpret_cast<const f32x4 *>(p.scale + c0), sc_hi = *reinterpret_cast<const f32x4 *>(p.scale + c0 + 4);
  const f32x4 bi_lo = *reinterpret_cast<const f32x4 *>(p.bias + c0), bi_hi = *reinterpret_cast<const f32x4 *>(p.bias + c0 + 4);
  float v[8];
  y3_bn_act8(v, f32x4{acc[0], acc[1], acc[2], acc[3]}, f32x4{acc[4], acc[5], acc[6], acc[7]}, sc_lo, sc_hi, bi_lo, bi_hi, act);
  T *o = static_cast<T *>(p.out) + m * p.out_ld + c0;
  const T *r = static_cast<const T *>(p.res) + m * p.res_ld + c0;
  if (vec) {
    if (p.flags & Y3_F_RESIDUAL) {
      float rv[8];
      ld8<T>(r, rv);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += rv[i];
    }
    st8<T>(o, v);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (p.flags & Y3_F_RESIDUAL) v[i] += y3_to_float<T>(r[i]);
      o[i] = y3_from_float<T>(v[i]);
    }
  }
}

// Eight channels as four float pairs: with -ffp-contract=off a pair's product and sum compile to v_pk_mul_f32 and v_pk_add_f32,
// each rounding as the scalar instruction does, at half the instruction count.
struct F8 {
  f32x2 q[4];
};
template <typename T>
__device__ __forceinline__ F8 ld8p(const T *p) {
  float v[8];
  ld8<T>(p, v);
  return F8{{f32x2{v[0], v[1]}, f32x2{v[2], v[3]}, f32x2{v[4], v[5]}, f32x2{v[6], v[7]}}};
}
// ... of an input column that may lie outside the row: the load goes to the nearest column inside (no branch around it, so a
// row's loads are all in flight together) and a column outside reads as +0.0.  Its products are zeros and leave every sum as it
// is (a sum that starts at +0.0 never holds -0.0; weights are finite), which is what skipping the tap gives.
template <typename T>
__device__ __forceinline__ F8 ld8p_col(const T *row, int ix, int W, int in_ld) {
  const bool ok = (unsigned)ix < (unsigned)W;
  const int ic = ix < 0 ? 0 : (ix >= W ? W - 1 : ix);
  const T *p = row + (long long)ic * in_ld;
  if constexpr (sizeof(T) == 4) {
    f32x4 a = *reinterpret_cast<const f32x4 *>(p), b = *reinterpret_cast<const f32x4 *>(p + 4);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    a = ok ? a : z;
    b = ok ? b : z;
    return F8{{f32x2{a[0], a[1]}, f32x2{a[2], a[3]}, f32x2{b[0], b[1]}, f32x2{b[2], b[3]}}};
  } else {
    u32x4 raw = *reinterpret_cast<const u32x4 *>(p);
    const u32x4 z = {0u, 0u, 0u, 0u};
    raw = ok ? raw : z;
    float v[8];
    y3_unpack8<T>(v, raw);
    return F8{{f32x2{v[0], v[1]}, f32x2{v[2], v[3]}, f32x2{v[4], v[5]}, f32x2{v[6], v[7]}}};
  }
}
__device__ __forceinline__ void mac8(F8 &acc, const F8 &x, const F8 &w) {
#pragma unroll
  for (int q = 0; q < 4; ++q) acc.q[q] += x.q[q] * w.q[q];
}

// KS > 0: ksize KS and stride S, weights in registers; KS == 0: ksize and stride of the op, weights read per tap
template <typename T, int KS, int S>
__global__ __launch_bounds__(256) void conv_dwise_kernel(GroupedArgs p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  const int c0 = (int)(idx % p.nchunk) * 8;
  int r = (int)(idx / p.nchunk);
  const int ox0 = (r % p.nxr) * kDwRun;
  r /= p.nxr;
  const int oy = r % p.Ho, b = r / p.Ho;
  const int ks = KS ? KS : p.ks, stride = KS ? S : p.stride;
  const int ix0 = ox0 * stride - p.pad, iy0 = oy * stride - p.pad;
  const T *wp = static_cast<const T *>(p.wgt) + c0;      // [ks * ks][k_ld], this lane's chunk
  F8 w[KS ? KS * KS : 1];
  if constexpr (KS > 0) {
#pragma unroll
    for (int t = 0; t < KS * KS; ++t) w[t] = ld8p<T>(wp + t * p.k_ld);
  }
  F8 acc[kDwRun];
#pragma unroll
  for (int j = 0; j < kDwRun; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[j].q[q] = f32x2{0.f, 0.f};
  // Per output the taps are visited ky outermost, kx ascending: a column ix serves output j as tap kx = ix - (ox0 + j) * stride
  // + pad, and the columns ascend.  Rows outside the image are skipped.
  if constexpr (KS > 0) {
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
      const int iy = iy0 + ky;
      if ((unsigned)iy >= (unsigned)p.H) continue;
      const T *row = static_cast<const T *>(p.in) + ((long long)b * p.H + iy) * p.W * p.in_ld + c0;
      constexpr int NCOL = (kDwRun - 1) * S + KS;
      F8 x[NCOL];
#pragma unroll
      for (int ci = 0; ci < NCOL; ++ci) x[ci] = ld8p_col<T>(row, ix0 + ci, p.W, p.in_ld);
#pragma unroll
      for (int ci = 0; ci < NCOL; ++ci) {
#pragma unroll
        for (int j = 0; j < kDwRun; ++j) {
          const int kx = ci - j * S;
          if (kx >= 0 && kx < KS) mac8(acc[j], x[ci], w[ky * KS + kx]);
        }
      }
    }
  } else {
    const int ncol = (kDwRun - 1) * stride + ks;
    for (int ky = 0; ky < ks; ++ky) {
      const int iy = iy0 + ky;
      if ((unsigned)iy >= (unsigned)p.H) continue;
      const T *row = static_cast<const T *>(p.in) + ((long long)b * p.H + iy) * p.W * p.in_ld + c0;
      for (int ci = 0; ci < ncol; ++ci) {
        const F8 x = ld8p_col<T>(row, ix0 + ci, p.W, p.in_ld);
#pragma unroll
        for (int j = 0; j < kDwRun; ++j) {
          const int kx = ci - j * stride;
          if (kx >= 0 && kx < ks) mac8(acc[j], x, ld8p<T>(wp + (ky * ks + kx) * p.k_ld));
        }
      }
    }
  }
  const int act = y3_act(p.flags);
  const long long m0 = ((long long)b * p.Ho + oy) * p.Wo + ox0;
#pragma unroll
  for (int j = 0; j < kDwRun; ++j)
    if (ox0 + j < p.Wo) {
      const float a[8] = {acc[j].q[0][0], acc[j].q[0][1], acc[j].q[1][0], acc[j].q[1][1],
                          acc[j].q[2][0], acc[j].q[2][1], acc[j].q[3][0], acc[j].q[3][1]};
      epilogue8<T>(p, a, m0 + j, c0, act, true);
    }
}

// OC == 8: eight consecutive output channels (all of one group: Cout / groups is a multiple of 8) of one pixel per thread;
// OC == 1: one output element per thread
template <typename T, int OC>
__global__ __launch_bounds__(256) void conv_grouped_kernel(GroupedArgs p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  const int nco = p.Cout / OC;
  const int co = (int)(idx % nco) * OC;
  const long long m = idx / nco;
  const int hw = p.Ho * p.Wo;
  const int b = (int)(m / hw);
  const int rem = (int)(m - (long long)b * hw);
  const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
  const int cg_in = p.Cin / p.groups, cg_out = p.Cout / p.groups;
  const int ci0 = (co / cg_out) * cg_in;                                   // the group's first input channel
  const T *w = static_cast<const T *>(p.wgt) + (long long)co * p.k_ld;     // [cout_pad][k_ld], k = (ky * ks + kx) * cg_in + c
  float acc[OC];
#pragma unroll
  for (int o = 0; o < OC; ++o) acc[o] = 0.f;
  for (int ky = 0; ky < p.ks; ++ky) {
    const int iy = oy * p.stride - p.pad + ky;
    if ((unsigned)iy >= (unsigned)p.H) continue;
    for (int kx = 0; kx < p.ks; ++kx) {
      const int ix = ox * p.stride - p.pad + kx;
      if ((unsigned)ix >= (unsigned)p.W) continue;
      const T *xp = static_cast<const T *>(p.in) + (((long long)b * p.H + iy) * p.W + ix) * p.in_ld + ci0;
      const T *wk = w + (ky * p.ks + kx) * cg_in;
      if (OC == 8 && p.vec_in) {
        for (int c = 0; c < cg_in; c += 8) {
          float x[8];
          ld8<T>(xp + c, x);
#pragma unroll
          for (int o = 0; o < OC; ++o) {
            float wv[8];
            ld8<T>(wk + (long long)o * p.k_ld + c, wv);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[o] += x[e] * wv[e];
          }
        }
      } else {
        for (int c = 0; c < cg_in; ++c) {
          const float x = y3_to_float<T>(xp[c]);
#pragma unroll
          for (int o = 0; o < OC; ++o) acc[o] += x * y3_to_float<T>(wk[(long long)o * p.k_ld + c]);
        }
      }
    }
  }
  const int act = y3_act(p.flags);
  if constexpr (OC == 8) {
    epilogue8<T>(p, acc, m, co, act, p.vec_out != 0);
  } else {
    float v = y3_bn_act1(acc[0], p.scale[co], p.bias[co], act);
    if (p.flags & Y3_F_RESIDUAL) v += y3_to_float<T>(static_cast<const T *>(p.res)[m * p.res_ld + co]);
    static_cast<T *>(p.out)[m * p.out_ld + co] = y3_from_float<T>(v);
  }
}

bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

GroupedArgs grouped_args(const y3_op &op, const void *d_in) {
  GroupedArgs a;
  a.in = d_in; a.wgt = op.d_weight; a.scale = op.d_scale; a.bias = op.d_bias; a.res = op.d_res; a.out = op.d_out;
  a.B = op.batch; a.H = op.in_h; a.W = op.in_w; a.Cin = op.in_c; a.in_ld = op.in_ld;
  a.Ho = op.out_h; a.Wo = op.out_w; a.Cout = op.out_c; a.out_ld = op.out_ld; a.res_ld = op.res_ld;
  a.ks = op.ksize; a.stride = op.stride; a.pad = op.pad; a.k_ld = op.k_ld; a.groups = op.groups;
  a.nchunk = op.out_c / 8;
  a.nxr = y3_ceil_div(op.out_w, kDwRun);
  a.vec_in = a.vec_out = 0;
  a.total = 0;
  a.flags = op.flags;
  return a;
}

// the depthwise instance of an op: 1 / 2 = 3x3 with stride 1 / 2 (weights in registers), 0 = any size and stride
int dwise_variant(const y3_op &op) { return op.ksize == 3 && (op.stride == 1 || op.stride == 2) ? op.stride : 0; }
long long dwise_threads(const y3_op &op) {
  return (long long)op.batch * op.out_h * y3_ceil_div(op.out_w, kDwRun) * (op.out_c / 8);
}
// output channels per thread of conv_grouped (the eight-channel form reads scale and bias with 16-byte loads)
int grouped_oc(const y3_op &op) { return (op.out_c / op.groups) % 8 == 0 && aligned16(op.d_scale) && aligned16(op.d_bias) ? 8 : 1; }

int launch_conv_dwise(const y3_op *ops, const y3_step &st, const void *d_in, const void *, hipStream_t s) {
  const y3_op &op = ops[0];
  GroupedArgs a = grouped_args(op, d_in);
  a.total = dwise_threads(op);
  return y3_by_dtype(op.dtype, [&](auto tag) {
    typedef decltype(tag) T;
    if (st.version == 1) return y3_launch<conv_dwise_kernel<T, 3, 1>>(st.dims, s, a);
    if (st.version == 2) return y3_launch<conv_dwise_kernel<T, 3, 2>>(st.dims, s, a);
    return y3_launch<conv_dwise_kernel<T, 0, 0>>(st.dims, s, a);
  });
}

int launch_conv_grouped(const y3_op *ops, const y3_step &st, const void *d_in, const void *, hipStream_t s) {
  const y3_op &op = ops[0];
  GroupedArgs a = grouped_args(op, d_in);
  const int cg_in = op.in_c / op.groups;
  a.total = (long long)op.batch * op.out_h * op.out_w * (op.out_c / st.bn);
  // (channel offsets of the plan's tensors are on the 8-channel grain, so the base addresses decide for every pixel)
  a.vec_in = cg_in % 8 == 0 && op.in_ld % 8 == 0 && op.k_ld % 8 == 0 && aligned16(d_in) && aligned16(op.d_weight);
  a.vec_out = op.out_ld % 8 == 0 && aligned16(op.d_out) && (!(op.flags & Y3_F_RESIDUAL) || (op.res_ld % 8 == 0 && aligned16(op.d_res)));
  return y3_by_dtype(op.dtype, [&](auto tag) {
    typedef decltype(tag) T;
    if (st.bn == 8) return y3_launch<conv_grouped_kernel<T, 8>>(st.dims, s, a);
    return y3_launch<conv_grouped_kernel<T, 1>>(st.dims, s, a);
  });
}

}  // namespace

// on the depthwise kernel's grain: one group per channel, everything a lane touches in whole 8-channel chunks at 16-byte aligned
// addresses (an address not set yet counts as aligned: the host asks y3_conv_path before it has laid the weights out).  An op
// off the grain, by a stride or by an address, is conv_grouped's.
bool y3_conv_dwise_fits(const y3_op &op) {
  const auto aligned = [](const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; };
  return op.kind == Y3_OP_CONV && op.groups > 1 && op.groups == op.in_c && op.in_c == op.out_c && op.in_c % 8 == 0 &&
         op.in_ld % 8 == 0 && op.out_ld % 8 == 0 && (!(op.flags & Y3_F_RESIDUAL) || (op.res_ld % 8 == 0 && aligned(op.d_res))) &&
         aligned(op.d_in) && aligned(op.d_out) && aligned(op.d_weight) && aligned(op.d_scale) && aligned(op.d_bias) &&
         !(op.flags & (Y3_F_IN_NCHW_F32 | Y3_F_IN_NHWC_U8BGR | Y3_F_PLAN_INPUT | Y3_F_OUT_F32));
}

int y3_choose_conv_dwise(const y3_op &op, y3_step &st) {
  Y3_REQUIRE(y3_conv_dwise_fits(op), "conv block %d: not a shape for the depthwise kernel", op.block_idx);
  Y3_REQUIRE(op.k_ld >= op.out_c && op.k_ld % 8 == 0 && op.cout_pad >= op.out_c, "conv block %d: depthwise weights need k_ld %% 8 == 0, k_ld and cout_pad >= %d",
             op.block_idx, op.out_c);
  st.launch = launch_conv_dwise;
  st.version = dwise_variant(op);
  st.dims = {y3_ceil_div64(dwise_threads(op), 256), 256, 0};   // one lane per 8-channel chunk of a run of kDwRun output pixels
  st.name = st.version == 1 ? Y3_KNAME(op.dtype, "conv_dwise_", "_k3s1")
                            : (st.version == 2 ? Y3_KNAME(op.dtype, "conv_dwise_", "_k3s2") : Y3_KNAME(op.dtype, "conv_dwise_", "_kn"));
  return Y3_OK;
}

int y3_choose_conv_grouped(const y3_op &op, y3_step &st) {
  Y3_REQUIRE(y3_is_grouped(op) && op.in_c % op.groups == 0 && op.out_c % op.groups == 0, "conv block %d: not a grouped conv", op.block_idx);
  Y3_REQUIRE((long long)op.k_ld >= (long long)op.ksize * op.ksize * (op.in_c / op.groups) && op.cout_pad >= op.out_c,
             "conv block %d: k_ld or cout_pad too small", op.block_idx);
  Y3_REQUIRE(!(op.flags & (Y3_F_IN_NCHW_F32 | Y3_F_IN_NHWC_U8BGR | Y3_F_PLAN_INPUT | Y3_F_OUT_F32)),
             "conv block %d: the grouped kernel reads and writes activations of the op's dtype only", op.block_idx);
  st.launch = launch_conv_grouped;
  st.bn = grouped_oc(op);
  st.dims = {y3_ceil_div64((long long)op.batch * op.out_h * op.out_w * (op.out_c / st.bn), 256), 256, 0};
  st.name = st.bn == 8 ? Y3_KNAME(op.dtype, "conv_grouped_", "_oc8") : Y3_KNAME(op.dtype, "conv_grouped_", "_oc1");
  return Y3_OK;
}
