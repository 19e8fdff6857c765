// Attention blocks of the Darknet cfgs (libyolov3_hip_attn.so): [avgpool] (global average pool), [scale_channels] and [sam].
// Memory-bound NHWC kernels in the manner of layers.hip: every tensor has a pixel stride (in_ld / res_ld / out_ld) because inputs
// and outputs live inside route-concat buffers, and each kernel has a 16-byte form (VEC = 16 / sizeof(T): one thread per channel
// chunk) and an element form (VEC = 1) for channel counts, pixel strides or base addresses off the 16-byte grain.  Both forms
// give the same bits.  The numerics are stated in include/yolov3_hip.h (Y3_OP_AVGPOOL, Y3_OP_SCALE_CHANNELS, Y3_OP_SAM).
// Compiled with -ffp-contract=off (Makefile: STRICT) and hipcc's default, correctly rounded float32 division.
#include "common.h"

namespace {

template <typename T, int VEC>
__device__ __forceinline__ void ld_vec(const T *p, float (&out)[VEC]) {
  if constexpr (VEC == 1) {
    out[0] = y3_to_float<T>(*p);
  } else {
    const u32x4 raw = *reinterpret_cast<const u32x4 *>(p);
    if constexpr (sizeof(T) == 4) {
      const f32x4 f = __builtin_bit_cast(f32x4, raw);
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = f[j];
    } else {
      y3_unpack8<T>(out, raw);
    }
  }
}

template <typename T, int VEC>
__device__ __forceinline__ void st_vec(T *p, const float (&in)[VEC]) {
  if constexpr (VEC == 1) {
    *p = y3_from_float<T>(in[0]);
  } else if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<f32x4 *>(p) = f32x4{in[0], in[1], in[2], in[3]};
  } else {
    *reinterpret_cast<u32x4 *>(p) = y3_pack8<T>(in);
  }
}

// ---- [avgpool] ------------------------------------------------------------------------------------------------------------
// out[b][c] = round_to_storage(S / float32(P)), P = H * W, S the float32 sum of the frame's P values of channel c in ONE order,
// a function of P alone (include/yolov3_hip.h):
//   32 partial sums start at +0.0f; partial r adds pixels r, r + 32, r + 64, ... in increasing order;
//   then s[r] += s[r + 16] for r < 16, and the same with 8, 4, 2, 1.
// One workgroup = one frame x kAvgCols neighbouring channel chunks (VEC channels each): thread t takes column t % kAvgCols and
// partial t / kAvgCols, so the kAvgCols lanes of one partial read consecutive 16-byte chunks of ONE pixel (128 contiguous bytes
// in the 16-byte form) and a wave reads eight pixels 32 apart.  The pixel loop is unrolled by kAvgUnroll: the loads of four
// pixels are in flight together and are then added in pixel order, so the unrolling does not show in the sum.  The tree runs in
// LDS (32 x kAvgCols x VEC floats, at most 8 KiB).  No atomics: the sum of a channel never leaves its workgroup.
constexpr int kAvgRows = 32, kAvgCols = 8, kAvgUnroll = 4;

struct AvgArgs {
  const void *in;
  void *out;
  int P, C, in_ld, out_ld, col_groups;   // col_groups = ceil(C / VEC / kAvgCols) workgroups per frame
};

template <typename T, int VEC>
__global__ __launch_bounds__(kAvgRows *kAvgCols) void avgpool_kernel(AvgArgs p) {
  __shared__ float part[kAvgRows][kAvgCols][VEC];
  const int col = threadIdx.x % kAvgCols, r = threadIdx.x / kAvgCols;
  const int b = blockIdx.x / p.col_groups, g = blockIdx.x - b * p.col_groups;
  const int c0 = (g * kAvgCols + col) * VEC;
  const bool live = c0 < p.C;                       // (C % VEC == 0 in the 16-byte form: a live chunk is a whole one)
  float s[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s[j] = 0.0f;
  if (live) {
    const T *base = static_cast<const T *>(p.in) + (long long)b * p.P * p.in_ld + c0;
    int px = r;
    for (; px + (kAvgUnroll - 1) * kAvgRows < p.P; px += kAvgUnroll * kAvgRows) {
      float v[kAvgUnroll][VEC];
#pragma unroll
      for (int u = 0; u < kAvgUnroll; ++u) ld_vec<T, VEC>(base + (long long)(px + u * kAvgRows) * p.in_ld, v[u]);
#pragma unroll
      for (int u = 0; u < kAvgUnroll; ++u)
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] += v[u][j];
    }
    for (; px < p.P; px += kAvgRows) {
      float v[VEC];
      ld_vec<T, VEC>(base + (long long)px * p.in_ld, v);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] += v[j];
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) part[r][col][j] = s[j];
  __syncthreads();
#pragma unroll
  for (int half = kAvgRows / 2; half >= 1; half >>= 1) {
    if (r < half) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) part[r][col][j] += part[r + half][col][j];
    }
    __syncthreads();
  }
  if (r == 0 && live) {
    const float n = (float)p.P;
    float o[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = part[0][col][j] / n;
    st_vec<T, VEC>(static_cast<T *>(p.out) + (long long)b * p.out_ld + c0, o);
  }
}

// ---- [scale_channels] and [sam] -------------------------------------------------------------------------------------------
// out = round_to_storage(float32(src) * float32(prev)): prev is (C, 1, 1) per frame for scale_channels (BCAST) and of src's shape
// for sam.  One thread per 16-byte chunk (or element) of the output, as add_kernel of layers.hip.
struct MulArgs {
  const void *prev, *src;
  void *out;
  int HW, C, prev_ld, src_ld, out_ld;
  long long total;   // B * HW * (C / VEC)
};

template <typename T, int VEC, bool BCAST>
__global__ __launch_bounds__(256) void attn_mul_kernel(MulArgs p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  const int cgroups = p.C / VEC;
  const int c0 = (int)(idx % cgroups) * VEC;
  const long long pix = idx / cgroups;
  const long long ppix = BCAST ? pix / p.HW : pix;
  float a[VEC], x[VEC];
  ld_vec<T, VEC>(static_cast<const T *>(p.prev) + ppix * p.prev_ld + c0, a);
  ld_vec<T, VEC>(static_cast<const T *>(p.src) + pix * p.src_ld + c0, x);
#pragma unroll
  for (int j = 0; j < VEC; ++j) x[j] *= a[j];
  st_vec<T, VEC>(static_cast<T *>(p.out) + pix * p.out_ld + c0, x);
}

bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

// the 16-byte form: every channel count, pixel stride and base address the op touches on the 16-byte grain (layers.hip's
// layer_is_wide; no attention op reads the plan's input, so every address is known when the plan is created)
bool attn_is_wide(const y3_op &op) {
  const int vec = 16 / y3_elem_size(op.dtype);
  bool wide = op.in_c % vec == 0 && op.in_ld % vec == 0 && op.out_ld % vec == 0 && aligned16(op.d_in) && aligned16(op.d_out);
  if (op.kind != Y3_OP_AVGPOOL) wide = wide && op.res_ld % vec == 0 && aligned16(op.d_res);
  return wide;
}

long long avg_col_groups(const y3_op &op, bool wide) {
  const int vec = wide ? 16 / y3_elem_size(op.dtype) : 1;
  return y3_ceil_div(y3_ceil_div(op.in_c, vec), kAvgCols);
}

int launch_avgpool(const y3_op *ops, const y3_step &st, const void *d_in, const void *, hipStream_t s) {
  const y3_op &op = ops[0];
  AvgArgs a;
  a.in = d_in; a.out = op.d_out;
  a.P = op.in_h * op.in_w; a.C = op.in_c; a.in_ld = op.in_ld; a.out_ld = op.out_ld;
  a.col_groups = (int)avg_col_groups(op, st.version == 1);
  return y3_by_dtype(op.dtype, [&](auto tag) {
    typedef decltype(tag) T;
    if (st.version == 1) return y3_launch<avgpool_kernel<T, 16 / sizeof(T)>>(st.dims, s, a);
    return y3_launch<avgpool_kernel<T, 1>>(st.dims, s, a);
  });
}

int launch_mul(const y3_op *ops, const y3_step &st, const void *d_in, const void *, hipStream_t s) {
  const y3_op &op = ops[0];
  const int vec = st.version == 1 ? 16 / y3_elem_size(op.dtype) : 1;
  MulArgs a;
  a.prev = d_in; a.src = op.d_res; a.out = op.d_out;
  a.HW = op.out_h * op.out_w; a.C = op.out_c; a.prev_ld = op.in_ld; a.src_ld = op.res_ld; a.out_ld = op.out_ld;
  a.total = (long long)op.batch * a.HW * (op.out_c / vec);
  const bool bcast = op.kind == Y3_OP_SCALE_CHANNELS;
  return y3_by_dtype(op.dtype, [&](auto tag) {
    typedef decltype(tag) T;
    constexpr int V = 16 / sizeof(T);
    if (st.version == 1) return bcast ? y3_launch<attn_mul_kernel<T, V, true>>(st.dims, s, a) : y3_launch<attn_mul_kernel<T, V, false>>(st.dims, s, a);
    return bcast ? y3_launch<attn_mul_kernel<T, 1, true>>(st.dims, s, a) : y3_launch<attn_mul_kernel<T, 1, false>>(st.dims, s, a);
  });
}

}  // namespace

int y3_choose_attention(const y3_op &op, y3_step &st) {
  const char *what = op.kind == Y3_OP_AVGPOOL ? "avgpool" : (op.kind == Y3_OP_SCALE_CHANNELS ? "scale_channels" : "sam");
  Y3_REQUIRE(op.kind == Y3_OP_AVGPOOL || op.kind == Y3_OP_SCALE_CHANNELS || op.kind == Y3_OP_SAM, "op for block %d: kind %d is no attention op",
             op.block_idx, op.kind);
  Y3_REQUIRE(op.out_h > 0 && op.out_w > 0 && op.out_c > 0, "%s block %d: empty output shape", what, op.block_idx);
  Y3_REQUIRE(op.in_c == op.out_c, "%s block %d: channel count changes (%d in, %d out)", what, op.block_idx, op.in_c, op.out_c);
  Y3_REQUIRE(op.in_ld >= op.in_c && op.out_ld >= op.out_c, "%s block %d: pixel stride below the channel count (in %d < %d or out %d < %d)", what,
             op.block_idx, op.in_ld, op.in_c, op.out_ld, op.out_c);
  if (op.kind == Y3_OP_AVGPOOL) {
    Y3_REQUIRE(op.out_h == 1 && op.out_w == 1, "avgpool block %d: output shape mismatch (%d x %d; a global pool gives 1 x 1)", op.block_idx, op.out_h,
               op.out_w);
  } else {
    Y3_REQUIRE(op.d_res != nullptr, "%s block %d: no source tensor (d_res)", what, op.block_idx);
    Y3_REQUIRE(op.res_ld >= op.out_c, "%s block %d: pixel stride of the source below the channel count (%d < %d)", what, op.block_idx, op.res_ld,
               op.out_c);
    if (op.kind == Y3_OP_SCALE_CHANNELS)
      Y3_REQUIRE(op.in_h == 1 && op.in_w == 1, "scale_channels block %d: shape mismatch: the scale is %d x %d x %d, not %d x 1 x 1", op.block_idx,
                 op.in_c, op.in_h, op.in_w, op.out_c);
    else
      Y3_REQUIRE(op.in_h == op.out_h && op.in_w == op.out_w, "sam block %d: shape mismatch: %d x %d x %d times %d x %d x %d", op.block_idx, op.in_c,
                 op.in_h, op.in_w, op.out_c, op.out_h, op.out_w);
  }
  const bool wide = attn_is_wide(op);
  st.version = wide ? 1 : 0;
  if (op.kind == Y3_OP_AVGPOOL) {
    st.launch = launch_avgpool;
    st.dims = {(long long)op.batch * avg_col_groups(op, wide), kAvgRows * kAvgCols, 0};   // (static LDS only)
    st.name = Y3_KNAME(op.dtype, "avgpool_", "");
  } else {
    const int vec = wide ? 16 / y3_elem_size(op.dtype) : 1;
    st.launch = launch_mul;
    st.dims = {y3_ceil_div64((long long)op.batch * op.out_h * op.out_w * (op.out_c / vec), 256), 256, 0};
    st.name = op.kind == Y3_OP_SCALE_CHANNELS ? Y3_KNAME(op.dtype, "scale_channels_", "") : Y3_KNAME(op.dtype, "sam_", "");
  }
  return Y3_OK;
}
