// Four-lanes-per-box YOLO decode, shared by yolo_decode_kernel<4> (yolo_decode.hip) and the fused head kernel
// (conv_igemm.hip, DECODE = true): the bf16 networks' form of YOLOLayer.forward's per-box arithmetic
// (/root/reference/yolov3/darknet.py:86-116).  One definition, so the fused and the two-kernel paths give the same bits
// for the same logits.
//
// The four lanes of a box (adjacent lanes, sub = lane & 3) split the class range; maxima, exp-sums and the arg-max are
// combined with quad DPP moves.  Differences from the sequential float32 form (yolo_decode_kernel<1>, the parity path):
//   * the class exponentials are exp2(x * log2(e)) on the hardware instruction (v_exp_f32, ~1 ulp; the argument's
//     rounding adds |x| * 6e-8) instead of expf -- 80 of the 85 transcendentals of a box; the soft-max denominator is
//     then within ~1e-6 relative of the sequential loop's (tests/test_gpu_parity.py::
//     test_split_class_decode_matches_sequential_decode), far below the bf16 logits' own noise;
//   * the exp-sum is a tree of four partial sums;
//   * box coordinates, objectness and the final product keep expf and IEEE division: identical to the sequential form.
// With Y3_F_SCORES_DARKNET the class terms are Darknet's independent logistics, p_c = 1 / (1 + exp2(-t_c * log2(e))) on the same
// hardware instruction (no maximum, no sum); the arg-max is taken on those p_c and the score is p_best * objectness.
// The box tail is spread over the four lanes (sub 0: x, 1: y, 2: w + objectness, 3: h + best / sum) with selects
// instead of branches, so no lane idles while one lane does five exponentials and seven divisions.
#pragma once
#include <stddef.h>

#include "common.h"

__device__ __forceinline__ float y3_quad_xor1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float y3_quad_xor2(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
}
__device__ __forceinline__ int y3_quad_xor1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ int y3_quad_xor2(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true); }
// lane 3 of the quad -> every lane of the quad
__device__ __forceinline__ float y3_quad_from3(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xFF, 0xF, 0xF, true));
}

// Darknet's [yolo] scale_x_y s stretches the sigmoid of the centre offsets: sig * s - (s - 1) / 2, computed as
// t = sig * s + (-0.5 (s - 1)) with every operation rounded on its own.  s == 1 (YOLOv3) gives sig itself, bit for bit:
// sig * 1 is exact and adding -0 changes nothing.
__device__ __forceinline__ float y3_scale_xy(float sig, float s) {
#pragma clang fp contract(off)
  return sig * s + (-0.5f * (s - 1.0f));
}
// y3_op.scale_x_y as the kernels take it: 0 (a caller that zero-initialises the op) means 1
static inline float y3_op_scale_xy(const y3_op &op) { return op.scale_x_y == 0.0f ? 1.0f : op.scale_x_y; }

// The decode fields of a fused head kernel's arguments (IgemmArgs, DwArgs: their last member), from the Y3_OP_YOLO op that
// reads the head conv
struct Y3DecodeArgs {
  float *bbox, *prob;
  long long *cls;
  int anchors, attr, row_offset, rows_total;
  float net_w, net_h, sxy, aw[8], ah[8];
  int mode;         // Y3_DECODE_* bits of the YOLO op (in what was the struct's tail padding; was `new_coords`, 0 / 1)
};
static_assert(sizeof(Y3DecodeArgs) == 120 && offsetof(Y3DecodeArgs, anchors) == 24 && offsetof(Y3DecodeArgs, net_w) == 40 &&
              offsetof(Y3DecodeArgs, ah) == 84 && offsetof(Y3DecodeArgs, mode) == 116,
              "layout of the decode fields in the kernel arguments");
// How a YOLO op scores a box, from its flags.  Y3_F_NEW_COORDS: the inputs are probabilities, and that decode is Darknet's
// already -- Y3_F_SCORES_DARKNET changes nothing there, so it sets no bit.  Otherwise Y3_F_SCORES_DARKNET replaces the reference's
// soft-max over the class logits by Darknet's independent logistic per class.
#define Y3_DECODE_NEW_COORDS 1
#define Y3_DECODE_SCORES_DARKNET 2
static inline int y3_decode_mode(const y3_op &yolo) {
  if (yolo.flags & Y3_F_NEW_COORDS) return Y3_DECODE_NEW_COORDS;
  return (yolo.flags & Y3_F_SCORES_DARKNET) ? Y3_DECODE_SCORES_DARKNET : 0;
}
static inline Y3DecodeArgs y3_decode_args(const y3_op &yolo) {
  Y3DecodeArgs d;
  d.bbox = yolo.d_bbox; d.prob = yolo.d_prob; d.cls = reinterpret_cast<long long *>(yolo.d_cls);
  d.anchors = yolo.n_anchor; d.attr = yolo.n_attr;
  d.row_offset = yolo.row_offset; d.rows_total = yolo.rows_total;
  d.net_w = yolo.net_w; d.net_h = yolo.net_h;
  d.sxy = y3_op_scale_xy(yolo);
  for (int i = 0; i < 8; ++i) { d.aw[i] = yolo.anchor_w[i]; d.ah[i] = yolo.anchor_h[i]; }
  d.mode = y3_decode_mode(yolo);
  return d;
}

// t_: the box's n_attr logits (LDS).  Called by all four lanes of the box together (EXEC must hold whole quads).
// cell_*: grid column / row of the box's cell; grid_*: grid size; anchor_*: the box's anchor (pixels); net_*: the network
// input size the anchors refer to; sxy: the head's scale_x_y; mode: Y3_DECODE_* bits, uniform over the launch (every branch on
// them is a scalar branch).  Y3_DECODE_NEW_COORDS: the inputs are the head conv's sigmoid outputs; centre (sxy(t) + cell) / grid, size
// ((t * t) * 4) * anchor / net, score best * t4, cls the first index of the largest stored class value.  Y3_DECODE_SCORES_DARKNET:
// the box as without it, score sigmoid(t_best) * sigmoid(t4), cls the first index of the largest class sigmoid.  (Scalars by value:
// selecting between members of a struct in memory by lane turns into an indexed load from scratch memory.)
// comp: this lane's box component (sub 0: bx, 1: by, 2: bw, 3: bh); score / cls are valid on the lane with sub == 2.
__device__ __forceinline__ void y3_decode_box4(const float *t_, int n_attr, int sub, float cell_x, float cell_y, float grid_w,
                                               float grid_h, float anchor_w, float anchor_h, float net_w, float net_h,
                                               float sxy, int mode, float &comp, float &score, int &cls) {
#pragma clang fp contract(off)
  constexpr float kLog2e = 1.44269504088896340736f;
  const int ncls = n_attr - 5;
  const int per = (ncls + 3) >> 2;
  const int c_lo = sub * per;
  float mx = -INFINITY, sum = 0.f, best = -1.f;
  int best_c = 0;
  const bool newc = (mode & Y3_DECODE_NEW_COORDS) != 0, dark = (mode & Y3_DECODE_SCORES_DARKNET) != 0;
  if (newc) {
    // the class values are probabilities already: compare them as stored.  (A max over the logits followed by one sigmoid
    // would not be the same arg-max: distinct logits above ~17 all give 1.0f, and the first of those must win.)
    const int c_hi = c_lo + per < ncls ? c_lo + per : ncls;
    for (int c = c_lo; c < c_hi; ++c) {
      const float v = t_[5 + c];
      if (v > best) {
        best = v;
        best_c = c;
      }
    }
  } else if (dark) {
    // Darknet's logistic per class.  The arg-max is taken on the probabilities as computed, as in the new_coords decode: distinct
    // logits above ~17 all give 1.0f and the first of them must win.
    const int c_hi = c_lo + per < ncls ? c_lo + per : ncls;
    for (int c = c_lo; c < c_hi; ++c) {
      const float v = 1.0f / (1.0f + __builtin_amdgcn_exp2f(-t_[5 + c] * kLog2e));
      if (v > best) {
        best = v;
        best_c = c;
      }
    }
  } else if (ncls == 80) {
    // COCO heads: the lane's 20 logits stay in registers between the two passes
    float v[20];
#pragma unroll
    for (int c = 0; c < 20; ++c) v[c] = t_[5 + c_lo + c];
#pragma unroll
    for (int c = 0; c < 20; ++c) mx = fmaxf(mx, v[c]);
    mx = fmaxf(mx, y3_quad_xor1(mx));
    mx = fmaxf(mx, y3_quad_xor2(mx));
#pragma unroll
    for (int c = 0; c < 20; ++c) {
      const float e = __builtin_amdgcn_exp2f((v[c] - mx) * kLog2e);
      sum += e;
      if (e > best) {  // strict: first index wins ties, like torch.max
        best = e;
        best_c = c_lo + c;
      }
    }
  } else {
    const int c_hi = c_lo + per < ncls ? c_lo + per : ncls;
    for (int c = c_lo; c < c_hi; ++c) mx = fmaxf(mx, t_[5 + c]);
    mx = fmaxf(mx, y3_quad_xor1(mx));
    mx = fmaxf(mx, y3_quad_xor2(mx));
    for (int c = c_lo; c < c_hi; ++c) {
      const float e = __builtin_amdgcn_exp2f((t_[5 + c] - mx) * kLog2e);
      sum += e;
      if (e > best) {
        best = e;
        best_c = c;
      }
    }
  }
  {
    const float os = y3_quad_xor1(sum), ob = y3_quad_xor1(best);
    const int oc = y3_quad_xor1(best_c);
    sum += os;                                       // both partners add the same two numbers: same result
    if (ob > best || (ob == best && oc < best_c)) {  // lower class index wins ties
      best = ob;
      best_c = oc;
    }
  }
  {
    const float os = y3_quad_xor2(sum), ob = y3_quad_xor2(best);
    const int oc = y3_quad_xor2(best_c);
    sum += os;
    if (ob > best || (ob == best && oc < best_c)) {
      best = ob;
      best_c = oc;
    }
  }
  // box component of this lane: sub 0 / 1: (sigmoid(t) * s - (s - 1) / 2 + cell) / grid;  sub 2 / 3: exp(t) * anchor / net
  const bool is_xy = (sub & 2) == 0, second = (sub & 1) != 0;
  const float tk = t_[sub];
  const float e = expf(is_xy ? -tk : tk);
  const float sig = 1.0f / (1.0f + e);
  const float cell = second ? cell_y : cell_x;
  const float anchor = second ? anchor_h : anchor_w;
  const float grid = second ? grid_h : grid_w;
  const float net = second ? net_h : net_w;
  const float num = is_xy ? y3_scale_xy(newc ? tk : sig, sxy) + cell : (newc ? ((tk * tk) * 4.0f) * anchor : e * anchor);
  const float den = is_xy ? grid : net;
  comp = num / den;
  // sub 2: objectness = sigmoid(t4);  sub 3: best / sum;  score = (best / sum) * objectness on sub 2
  // (new_coords: objectness = t4, sub 3: best, score = best * t4;  Darknet scores: sub 3: best, a probability already)
  const float e4 = expf(-t_[4]);
  const float den3 = dark ? 1.0f : sum;            // (best / 1.0f is best, exactly)
  const float r = newc ? (sub == 3 ? best : t_[4]) : (sub == 3 ? best : 1.0f) / (sub == 3 ? den3 : 1.0f + e4);
  const float q = y3_quad_from3(r);
  score = q * r;
  cls = best_c;
}

// YOLO decode of `rows` pixels whose float32 logits (conv sums with scale / bias already applied) are parked in LDS with
// a row stride of LD floats (LD odd in units of banks: the per-box reads of adjacent lanes spread over the banks): four
// lanes per box, y3_decode_box4 above -- the same code as yolo_decode_kernel<4>.  Args: the launch arguments of a fused head kernel
// (conv_igemm.hip: IgemmArgs, conv_1x1.hip: DwArgs) -- M, HoWo, Wo, Ho, the fast-division constants and the decode fields `dec`.
template <int NT, int LD, typename Args>
__device__ __forceinline__ void y3_head_decode_rows(const Args &p, const float *sL, int mbase, int rows, int tid) {
  const Y3DecodeArgs &d = p.dec;
  const int nbox = rows * d.anchors;
  const uint32_t inv_a = (65536u + (uint32_t)d.anchors - 1u) / (uint32_t)d.anchors;   // box / anchors for box < 8192
  for (int t = tid; t < nbox * 4; t += NT) {
    const int box = t >> 2, sub = t & 3;
    const int pl = (int)(((uint32_t)box * inv_a) >> 16), a = box - pl * d.anchors;
    const long long m = (long long)mbase + pl;
    const bool live = m < p.M;
    const uint32_t um = (uint32_t)(live ? m : p.M - 1);
    const uint32_t b = (__umulhi(um, p.mul_hw) + um) >> p.sh_hw;
    const uint32_t rem = um - b * (uint32_t)p.HoWo;
    const uint32_t y = (__umulhi(rem, p.mul_w) + rem) >> p.sh_w;
    const uint32_t x = rem - y * (uint32_t)p.Wo;
    float comp, score;
    int best_c;
    y3_decode_box4(sL + pl * LD + a * d.attr, d.attr, sub, (float)x, (float)y, (float)p.Wo, (float)p.Ho, d.aw[a], d.ah[a],
                   d.net_w, d.net_h, d.sxy, d.mode, comp, score, best_c);
    if (!live) continue;
    const long long row = (long long)b * d.rows_total + d.row_offset + (long long)a * p.HoWo + (long long)y * p.Wo + x;
    d.bbox[row * 4 + sub] = comp;
    if (sub == 2) {
      d.prob[row] = score;
      d.cls[row] = best_c;
    }
  }
}
