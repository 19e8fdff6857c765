// Darknet's multi-label candidates on device (get_yolo_detections): every class of a box whose score obj * p_c passes the
// threshold becomes a candidate ("virtual row") of its own, in ascending (row, class) order.  Not in the reference, whose
// YOLOLayer.forward keeps the arg-max class only (/root/reference/yolov3/darknet.py:104-108).  include/yolov3_hip.h states the
// rule; the arithmetic is the sequential form of Y3_F_SCORES_DARKNET (yolo_decode.hip), so in a float32 network a row's best
// label carries the decode's score bit for bit.  Built with -ffp-contract=off.
//
// Shape: a wave owns 64 consecutive prediction rows of one frame (a workgroup 256, a frame ceil(rows / 256) workgroups).
//   1. every lane reads the objectness of its own row -- one float of the box's n_attr -- and the wave ballots obj > thresh;
//   2. for each row that passed, in row order, the WHOLE wave reads that box's class values: they are contiguous, so a load is
//      one coalesced run of 64 floats; lane = class (mod 64), a ballot of s_c > thresh gives every label its slot inside the
//      wave by a population count of the lower lanes -- (row, class) order by construction, whatever the scheduling.
// Rows that fail the objectness test never touch their class values (at Darknet's 0.25 that is nearly all of them).
// Two launches of the same code: the first only counts, one counter per wave; the second sums the counters of the waves before
// its own (a few hundred per frame, one coalesced read) for its first slot, runs the ballots again and writes.  The class
// values of the rows that passed are therefore read TWICE: the worst case (a threshold near 0) is two reads of the head tensors,
// not one.  ASSUMPTION, not measured (profiles/r09_darknet_scores.txt): the second read is served mostly by the L2 / Infinity
// Cache, which the 124 MB of yolov3's heads at 608 x 608 and batch 16 fit.  Keeping the labels of the first pass instead would
// need a staging buffer of rows x classes.  Likewise unmeasured: the serial walk over the rows that passed (up to 64 per wave
// at a threshold of 0.001) is a dependent chain of loads and ballots per wave.  The second launch also writes the padding
// slots and the frame's true count.  All stores are ordinary vector stores.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kLabelHeads = 8;          // head views per call (32 B each as kernel arguments)
constexpr int kLabelThreads = 256;
constexpr int kLabelWaves = kLabelThreads / 64;

struct LabelHead {
  const float *p;
  int hw, ld, n_attr, row_offset, rows, new_coords;
};

struct LabelArgs {
  LabelHead head[kLabelHeads];
  int n_heads, rows_total, cap, nwaves;   // nwaves: waves (64 rows each) per frame
  float thresh;
  const float *bbox;
  int *counts;                            // (batch, nwaves) labels per wave
  float *vbbox, *vprob;
  long long *vcls;
  int *vrow, *vcount;
};

// the n_attr floats of prediction row `row` of frame f, or nullptr for a row no head covers
__device__ __forceinline__ const float *label_box(const LabelArgs &a, int f, int row, int &ncls, bool &newc) {
  const float *box = nullptr;
  ncls = 0;
  newc = false;
#pragma unroll
  for (int i = 0; i < kLabelHeads; ++i) {
    if (i >= a.n_heads) break;
    const LabelHead &hd = a.head[i];
    const int r = row - hd.row_offset;
    if (r >= 0 && r < hd.rows) {
      const int an = r / hd.hw, px = r - an * hd.hw;
      box = hd.p + ((long long)f * hd.hw + px) * hd.ld + an * hd.n_attr;
      ncls = hd.n_attr - 5;
      newc = hd.new_coords != 0;
    }
  }
  return box;
}

__device__ __forceinline__ float label_logistic(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

template <bool EMIT>
__global__ __launch_bounds__(kLabelThreads) void expand_labels_kernel(LabelArgs a) {
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const int wv = blockIdx.x * kLabelWaves + (threadIdx.x >> 6);
  if (wv >= a.nwaves) return;           // (whole waves leave; the kernel has no barrier)
  int first = 0, total = 0;             // EMIT: labels of the frame before this wave's / in all of it
  if (EMIT) {
    const int *cnt = a.counts + (long long)f * a.nwaves;
    for (int i = lane; i < a.nwaves; i += 64) {
      const int c = cnt[i];
      total += c;
      first += i < wv ? c : 0;
    }
    total = wave_sum(total);
    first = wave_sum(first);
  }
  const int row0 = wv * 64;
  float obj = 0.f;
  bool pass = false;
  {
    int ncls;
    bool newc;
    const float *box = row0 + lane < a.rows_total ? label_box(a, f, row0 + lane, ncls, newc) : nullptr;
    if (box) {
      const float t4 = box[4];
      obj = newc ? t4 : label_logistic(t4);
      pass = obj > a.thresh;            // strict; false for a NaN
    }
  }
  unsigned long long todo = __ballot(pass);
  int n = 0;                            // labels of this wave so far (wave-uniform)
  while (todo) {
    const int src = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int row = row0 + src;         // wave-uniform: every lane looks at the same box
    int ncls;
    bool newc;
    const float *box = label_box(a, f, row, ncls, newc);
    const float o = __shfl(obj, src);
    for (int c0 = 0; c0 < ncls; c0 += 64) {
      const int c = c0 + lane;
      float s = 0.f;
      bool hit = false;
      if (c < ncls) {
        const float t = box[5 + c];
        s = o * (newc ? t : label_logistic(t));
        hit = s > a.thresh;
      }
      const unsigned long long hm = __ballot(hit);
      if (EMIT && hit) {
        const int k = first + n + __popcll(hm & ((1ull << lane) - 1ull));
        if (k < a.cap) {
          const long long slot = (long long)f * a.cap + k;
          *reinterpret_cast<f32x4 *>(a.vbbox + slot * 4) =
              *reinterpret_cast<const f32x4 *>(a.bbox + ((long long)f * a.rows_total + row) * 4);
          a.vprob[slot] = s;
          a.vcls[slot] = c;
          a.vrow[slot] = row;
        }
      }
      n += __popcll(hm);
    }
  }
  if (!EMIT) {
    if (lane == 0) a.counts[(long long)f * a.nwaves + wv] = n;
    return;
  }
  // padding slots of the frame, shared out over its waves; the frame's true count
  for (int k = (total < a.cap ? total : a.cap) + row0 + lane; k < a.cap; k += a.nwaves * 64) {
    const long long slot = (long long)f * a.cap + k;
    *reinterpret_cast<f32x4 *>(a.vbbox + slot * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    a.vprob[slot] = -1.0f;
    a.vcls[slot] = 0;
    a.vrow[slot] = -1;
  }
  if (wv == 0 && lane == 0) a.vcount[f] = total;
}

int label_waves(int rows_total) { return (rows_total + 63) / 64; }

}  // namespace

extern "C" size_t y3_expand_labels_workspace_bytes(int batch, int rows_total, int cap) {
  if (batch <= 0 || rows_total <= 0 || cap <= 0) return 0;
  return ((size_t)batch * label_waves(rows_total) * sizeof(int) + 255) / 256 * 256;
}

extern "C" int y3_expand_labels(const y3_head_view *heads, int n_heads, const float *d_bbox, int batch, int rows_total,
                                float thresh, int cap, void *d_ws, size_t ws_bytes, float *d_vbbox, float *d_vprob,
                                int64_t *d_vcls, int32_t *d_vrow, int32_t *d_vcount, void *stream) {
  Y3_REQUIRE(heads && d_bbox && d_ws && d_vbbox && d_vprob && d_vcls && d_vrow && d_vcount, "y3_expand_labels: null pointer argument");
  Y3_REQUIRE(n_heads >= 1 && n_heads <= kLabelHeads, "y3_expand_labels: 1..%d head views per call, got %d", kLabelHeads, n_heads);
  Y3_REQUIRE(batch > 0 && batch <= 65535 && rows_total > 0, "y3_expand_labels: batch (<= 65535) and rows_total must be positive");
  Y3_REQUIRE(thresh >= 0.0f && thresh < INFINITY, "y3_expand_labels: thresh must be finite and >= 0");
  Y3_REQUIRE(cap >= 1 && cap <= (1 << 30), "y3_expand_labels: cap must be 1 .. 2^30, got %d", cap);
  Y3_REQUIRE(((uintptr_t)d_bbox & 15) == 0 && ((uintptr_t)d_vbbox & 15) == 0, "y3_expand_labels: d_bbox and d_vbbox must be 16-byte aligned");
  Y3_REQUIRE(((uintptr_t)d_ws & 3) == 0 && ws_bytes >= y3_expand_labels_workspace_bytes(batch, rows_total, cap),
             "y3_expand_labels: workspace too small or misaligned");
  LabelArgs a = {};
  int max_attr = 0;
  for (int i = 0; i < n_heads; ++i) {
    const y3_head_view &v = heads[i];
    Y3_REQUIRE(v.d_head && v.h > 0 && v.w > 0 && v.n_anchor >= 1 && v.n_attr >= 6, "y3_expand_labels: head %d: null pointer or empty shape", i);
    const long long rows = (long long)v.n_anchor * v.h * v.w;
    Y3_REQUIRE((long long)v.n_anchor * v.n_attr <= v.ld, "y3_expand_labels: head %d: %d anchors x %d attributes exceed the pixel stride %d",
               i, v.n_anchor, v.n_attr, v.ld);
    Y3_REQUIRE(v.row_offset >= 0 && v.row_offset + rows <= rows_total, "y3_expand_labels: head %d: rows %d .. %lld outside 0 .. %d",
               i, v.row_offset, v.row_offset + rows, rows_total);
    for (int j = 0; j < i; ++j)
      Y3_REQUIRE(v.row_offset >= a.head[j].row_offset + a.head[j].rows || a.head[j].row_offset >= v.row_offset + rows,
                 "y3_expand_labels: heads %d and %d overlap in their rows", j, i);
    a.head[i] = LabelHead{v.d_head, v.h * v.w, v.ld, v.n_attr, v.row_offset, (int)rows, v.new_coords};
    max_attr = v.n_attr > max_attr ? v.n_attr : max_attr;
  }
  Y3_REQUIRE((long long)rows_total * max_attr <= INT_MAX - 64, "y3_expand_labels: %d rows x %d attributes: label count out of range",
             rows_total, max_attr);
  a.n_heads = n_heads;
  a.rows_total = rows_total;
  a.cap = cap;
  a.nwaves = label_waves(rows_total);
  a.thresh = thresh;
  a.bbox = d_bbox;
  a.counts = static_cast<int *>(d_ws);
  a.vbbox = d_vbbox;
  a.vprob = d_vprob;
  a.vcls = reinterpret_cast<long long *>(d_vcls);
  a.vrow = d_vrow;
  a.vcount = d_vcount;
  const dim3 grid((unsigned)((a.nwaves + kLabelWaves - 1) / kLabelWaves), (unsigned)batch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = y3_launch<expand_labels_kernel<false>>(grid, dim3(kLabelThreads), 0, s, a);
  if (rc != Y3_OK) return rc;
  return y3_launch<expand_labels_kernel<true>>(grid, dim3(kLabelThreads), 0, s, a);
}
