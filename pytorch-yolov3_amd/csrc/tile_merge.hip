// Seam merging for tiled frames (y3_merge_tiled, libyolov3_hip_tilemerge.so): the second, cross-tile pass that joins the partial
// boxes an object cut by a tile border leaves behind.  Not in the reference.  The rule is stated in include/yolov3_hip.h; in short:
// over one frame's detections in the canonical order of y3_detect_tiled, a detection that nothing has absorbed is a keeper, and a
// keeper absorbs every later detection of its class, from ANOTHER tile, not yet absorbed, whose box it matches; a matches b iff
// inter / min(area_a, area_b) > thr (intersection over the smaller area: +1 pixel convention, int64, one float64 division, strict).
// Matching always uses the original boxes; a keeper's output box is the union of its own and of everything it absorbed.
//
// One launch per batch, one 1024-thread workgroup per frame, phases separated by workgroup barriers:
//   1  class segments of the (already sorted) input -> work items in the workspace
//   2  every segment runs WHOLLY on one wave, in 64-detection chunks, one box per lane, as the chunk routine of detect.hip walks a
//      class: the keepers of the earlier chunks are broadcast by v_readlane, then a greedy pass inside the chunk; victims are taken
//      by a ballot mask and record their owner.  Segments are dealt to the 16 waves round robin.  No wave ever waits for another:
//      the only synchronisation of the kernel is the workgroup barrier (the flag chain of detect_kernel is not used here -- the
//      inputs are kept detections, tens to a few thousand).
//   3  ordered gather of the keepers (ballot prefix sums): own box, score, class, row, members = 1
//   4  every absorbed detection folds its original box into its owner's output box with integer atomic min / max (exact, and
//      independent of the order) and counts itself in the owner's members
// Two chunks whose boxes all lie within +-16000 are compared in 32-bit integers without a division where the sign of
// inter - thr * min_area decides; everything else takes int64 / float64.  Both give the stated rule exactly.
// Built with -ffp-contract=off.  LDS: 68 bytes (16 wave totals and the segment counter).
#include "common.h"

#include <limits.h>
#include <cmath>

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;

struct MergeArgs {
  // inputs: what y3_detect_tiled wrote
  const int *in_count;
  const long long *in_tlbr;
  const float *in_prob;
  const long long *in_cls;
  const int *in_row;
  int capacity;     // detections per frame, at most
  int tile_rows;
  double thr;
  // workspace, per frame
  int *owner;       // [capacity]  -1 = keeper, otherwise the index of the keeper that absorbed it
  int *slot;        // [capacity]  a keeper's position in the output
  int *items;       // [capacity][2]  class segments: start, end
  // outputs
  int *out_count;
  long long *out_tlbr;
  float *out_prob;
  long long *out_cls;
  int *out_row;
  int *out_members;  // may be null
};

// value of lane k (wave-uniform k) as a scalar: v_readlane_b32, no LDS traffic
__device__ __forceinline__ long long readlane_ll(long long v, int k) {
  const int lo = __builtin_amdgcn_readlane((int)(v & 0xFFFFFFFFll), k);
  const int hi = __builtin_amdgcn_readlane((int)(v >> 32), k);
  return ((long long)hi << 32) | (unsigned int)lo;
}

// One detection per lane: the int64 corners and area, their int32 copies, the tile, `ok` = inside the segment and not degenerate
// (w > 0 and h > 0), and the wave-uniform "every box of this chunk lies within +-16000" bit.
struct Box {
  long long x1, y1, x2, y2, area;
  int ix1, iy1, ix2, iy2, iarea;
  int tile;
  bool ok;
  bool fits;
};

__device__ __forceinline__ bool box_fits_i32(long long x1, long long y1, long long x2, long long y2) {
  const long long lim = 16000;
  return x1 > -lim && x1 < lim && y1 > -lim && y1 < lim && x2 > -lim && x2 < lim && y2 > -lim && y2 < lim;
}

// called by whole wavefronts (it ballots)
__device__ __forceinline__ Box load_box(bool valid, const long long *tlbr, const int *row, int idx, int tile_rows) {
  Box b;
  b.x1 = b.y1 = b.x2 = b.y2 = 0;
  b.tile = 0;
  if (valid) {
    const long long *bp = tlbr + (long long)idx * 4;
    b.x1 = bp[0]; b.y1 = bp[1]; b.x2 = bp[2]; b.y2 = bp[3];
    b.tile = row[idx] / tile_rows;
  }
  const long long w = b.x2 - b.x1 + 1, h = b.y2 - b.y1 + 1;
  // (unsigned products: a degenerate or far-away box that nobody asks about must not overflow a signed type)
  b.area = (long long)((unsigned long long)w * (unsigned long long)h);
  b.ok = valid && w > 0 && h > 0;
  b.fits = __ballot(box_fits_i32(b.x1, b.y1, b.x2, b.y2)) == ~0ull;
  b.ix1 = (int)b.x1; b.iy1 = (int)b.y1; b.ix2 = (int)b.x2; b.iy2 = (int)b.y2;
  b.iarea = (int)(((unsigned)b.ix2 - (unsigned)b.ix1 + 1u) * ((unsigned)b.iy2 - (unsigned)b.iy1 + 1u));   // exact where the chunk fits
  return b;
}

// Does lane k (wave-uniform, a non-degenerate box) of chunk `a` match my box?  Only lanes with me.ok use the answer; for them both
// areas are >= 1.  Called by whole wavefronts: it reads other lanes and ballots.
// narrow: widths <= 32001 and areas <= 1.03e9, exact in 32-bit integers.  fl(inter / m) > thr (m = the smaller area, float64 true
// division) is decided without dividing: d = inter - thr * m (one fma rounding) has the exact sign of inter / m - thr, and the
// rounded quotient can disagree with that sign only inside (thr, thr + ulp(thr) / 2]; pairs that close (0 < d <= m * thr * 2.3e-16)
// take the division.  thr_m = thr * 2.3e-16.
__device__ __forceinline__ bool matches(const Box &a, int k, const Box &me, bool narrow, double thr, double thr_m) {
  if (narrow) {
    const int ax1 = __builtin_amdgcn_readlane(a.ix1, k), ay1 = __builtin_amdgcn_readlane(a.iy1, k);
    const int ax2 = __builtin_amdgcn_readlane(a.ix2, k), ay2 = __builtin_amdgcn_readlane(a.iy2, k);
    const int aarea = __builtin_amdgcn_readlane(a.iarea, k);
    int iw = (ax2 < me.ix2 ? ax2 : me.ix2) - (ax1 > me.ix1 ? ax1 : me.ix1) + 1;
    int ih = (ay2 < me.iy2 ? ay2 : me.iy2) - (ay1 > me.iy1 ? ay1 : me.iy1) + 1;
    iw = iw > 0 ? iw : 0;
    ih = ih > 0 ? ih : 0;
    const int inter = iw * ih;
    const int m = aarea < me.iarea ? aarea : me.iarea;
    const double i = (double)inter, s = (double)m;
    const double d = fma(-thr, s, i);
    bool hit = d > s * thr_m;
    const bool unsure = me.ok && d > 0.0 && !hit;
    if (__ballot(unsure) != 0ull) {
      if (unsure) hit = i / s > thr;
    }
    return hit;
  }
  const long long ax1 = readlane_ll(a.x1, k), ay1 = readlane_ll(a.y1, k);
  const long long ax2 = readlane_ll(a.x2, k), ay2 = readlane_ll(a.y2, k);
  const long long aarea = readlane_ll(a.area, k);
  long long iw = (ax2 < me.x2 ? ax2 : me.x2) - (ax1 > me.x1 ? ax1 : me.x1) + 1;
  long long ih = (ay2 < me.y2 ? ay2 : me.y2) - (ay1 > me.y1 ? ay1 : me.y1) + 1;
  iw = iw > 0 ? iw : 0;
  ih = ih > 0 ? ih : 0;
  const long long inter = iw * ih;
  const long long m = aarea < me.area ? aarea : me.area;
  return (double)inter / (double)m > thr;
}

// block-wide ordered compaction step: returns this thread's output slot (valid when flag) and adds the step's total to
// `running`.  Must be called by all threads.
__device__ __forceinline__ int ordered_slot(bool flag, int &running, int *wave_tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long ballot = __ballot(flag);
  const int prefix = __popcll(ballot & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[wave] = __popcll(ballot);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int t = wave_tot[w];
    before += w < wave ? t : 0;
    total += t;
  }
  const int slot = running + before + prefix;
  running += total;
  __syncthreads();
  return slot;
}

__global__ __launch_bounds__(kThreads) void tile_merge_kernel(MergeArgs p) {
  __shared__ int wave_tot[kWaves];
  __shared__ int nitem_sh;

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const long long C = p.capacity;
  int n = p.in_count[b];
  n = n < 0 ? 0 : (n > p.capacity ? p.capacity : n);   // never past a buffer, whatever the count says
  if (n == 0) {
    if (tid == 0) p.out_count[b] = 0;
    return;
  }
  const long long *tlbr = p.in_tlbr + b * C * 4;
  const float *prob = p.in_prob + b * C;
  const long long *cls = p.in_cls + b * C;
  const int *row = p.in_row + b * C;
  int *owner = p.owner + b * C;
  int *slot_of = p.slot + b * C;
  int *items = p.items + b * C * 2;

  // ---- phase 1: class segments -> work items (the input is sorted by class: no sort) ------------------------------
  if (tid == 0) nitem_sh = 0;
  __syncthreads();
  for (int i = tid; i < n; i += kThreads) {
    const long long c = cls[i];
    if (i == 0 || cls[i - 1] != c) {
      int lo = i + 1, hi = n;  // first index in (i, n] whose class differs
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cls[mid] == c) lo = mid + 1; else hi = mid;
      }
      const int it = atomicAdd(&nitem_sh, 1);   // at most n <= capacity segments
      items[it * 2 + 0] = i;
      items[it * 2 + 1] = lo;
    }
  }
  __syncthreads();
  const int nitem = nitem_sh;

  // ---- phase 2: the greedy pass, one segment per wave at a time ------------------------------------------------------
  const double thr = p.thr, thr_m = p.thr * 2.3e-16;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int it = wave_u; it < nitem; it += kWaves) {
    const int start = __builtin_amdgcn_readfirstlane(items[it * 2 + 0]);
    const int end = __builtin_amdgcn_readfirstlane(items[it * 2 + 1]);
    const int nch = (end - start + 63) >> 6;
    for (int j = 0; j < nch; ++j) {
      const int idx = start + 64 * j + lane;
      const bool valid = idx < end;
      const Box me = load_box(valid, tlbr, row, idx, p.tile_rows);
      int mine = -1;   // my owner
      // keepers of the earlier chunks of this segment, in order.  owner[p0 + lane] was written by this very lane.
      for (int jj = 0; jj < j; ++jj) {
        if (__ballot(me.ok && mine < 0) == 0ull) break;           // nobody left to take
        const int p0 = start + 64 * jj;                           // an earlier chunk is full: p0 + lane < end
        const Box q = load_box(true, tlbr, row, p0 + lane, p.tile_rows);
        unsigned long long kept = __ballot(q.ok && owner[p0 + lane] < 0);
        const bool narrow = q.fits && me.fits;
        while (kept) {
          const int k = __ffsll((long long)kept) - 1;
          kept &= kept - 1ull;
          const bool hit = matches(q, k, me, narrow, thr, thr_m);   // by every lane: the test reads other lanes
          if (hit && me.ok && mine < 0 && me.tile != __builtin_amdgcn_readlane(q.tile, k)) mine = p0 + k;
        }
      }
      // greedy inside the chunk, in lane order; an absorbed lane leaves the candidates
      unsigned long long cand = __ballot(me.ok && mine < 0);
      for (int k = 0; k < 64; ++k) {
        if (!((cand >> k) & 1ull)) continue;  // wave-uniform
        const bool hit = matches(me, k, me, me.fits, thr, thr_m);
        const bool take = hit && lane > k && me.ok && mine < 0 && me.tile != __builtin_amdgcn_readlane(me.tile, k);
        if (take) mine = start + 64 * j + k;
        cand &= ~__ballot(take);
      }
      if (valid) owner[idx] = mine;
      __threadfence_block();  // later chunks of this wavefront read these owners
    }
  }
  __threadfence();
  __syncthreads();

  // ---- phase 3: ordered gather of the keepers -------------------------------------------------------------------------
  long long *o_tlbr = p.out_tlbr + b * C * 4;
  int *o_members = p.out_members ? p.out_members + b * C : nullptr;
  int kept_n = 0;
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + tid;
    const bool flag = i < n && owner[i] < 0;
    const int slot = ordered_slot(flag, kept_n, wave_tot);
    if (flag) {
      const long long *bp = tlbr + (long long)i * 4;
      long long *o = o_tlbr + (long long)slot * 4;
      o[0] = bp[0]; o[1] = bp[1]; o[2] = bp[2]; o[3] = bp[3];
      p.out_prob[b * C + slot] = prob[i];
      p.out_cls[b * C + slot] = cls[i];
      p.out_row[b * C + slot] = row[i];
      if (o_members) o_members[slot] = 1;
      slot_of[i] = slot;
    }
  }
  if (tid == 0) p.out_count[b] = kept_n;
  if (kept_n == n) return;   // nothing was absorbed (workgroup-uniform)
  __threadfence();
  __syncthreads();

  // ---- phase 4: unions and member counts --------------------------------------------------------------------------------
  for (int i = tid; i < n; i += kThreads) {
    const int k = owner[i];
    if (k < 0) continue;
    const long long *bp = tlbr + (long long)i * 4;
    const int slot = slot_of[k];
    long long *o = o_tlbr + (long long)slot * 4;
    __hip_atomic_fetch_min(o + 0, bp[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(o + 1, bp[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(o + 2, bp[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(o + 3, bp[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o_members) __hip_atomic_fetch_add(o_members + slot, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct WsLayout {
  size_t owner, slot, items, total;
};

WsLayout ws_layout(int batch, int capacity) {
  WsLayout w;
  const size_t n = (size_t)batch * (size_t)capacity;
  size_t off = 0;
  w.owner = off; off = align_up(off + n * sizeof(int));
  w.slot = off; off = align_up(off + n * sizeof(int));
  w.items = off; off = align_up(off + n * 2 * sizeof(int));
  w.total = off;
  return w;
}

bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" size_t y3_merge_tiled_workspace_bytes(int batch, int capacity) {
  if (batch <= 0 || capacity <= 0) return 0;
  return ws_layout(batch, capacity).total;
}

extern "C" int y3_merge_tiled(const int32_t *d_det_count, const int64_t *d_det_tlbr, const float *d_det_prob,
                              const int64_t *d_det_cls, const int32_t *d_det_row, int batch, int capacity, int tile_rows,
                              double thr, void *d_workspace, size_t workspace_bytes, int32_t *d_out_count, int64_t *d_out_tlbr,
                              float *d_out_prob, int64_t *d_out_cls, int32_t *d_out_row, int32_t *d_out_members, void *stream) {
  Y3_REQUIRE(d_det_count, "y3_merge_tiled: d_det_count is null");
  Y3_REQUIRE(d_det_tlbr, "y3_merge_tiled: d_det_tlbr is null");
  Y3_REQUIRE(d_det_prob, "y3_merge_tiled: d_det_prob is null");
  Y3_REQUIRE(d_det_cls, "y3_merge_tiled: d_det_cls is null");
  Y3_REQUIRE(d_det_row, "y3_merge_tiled: d_det_row is null");
  Y3_REQUIRE(d_workspace, "y3_merge_tiled: d_workspace is null");
  Y3_REQUIRE(d_out_count, "y3_merge_tiled: d_out_count is null");
  Y3_REQUIRE(d_out_tlbr, "y3_merge_tiled: d_out_tlbr is null");
  Y3_REQUIRE(d_out_prob, "y3_merge_tiled: d_out_prob is null");
  Y3_REQUIRE(d_out_cls, "y3_merge_tiled: d_out_cls is null");
  Y3_REQUIRE(d_out_row, "y3_merge_tiled: d_out_row is null");
  Y3_REQUIRE(batch >= 1, "y3_merge_tiled: batch must be positive (%d)", batch);
  Y3_REQUIRE(capacity >= 1, "y3_merge_tiled: capacity must be positive (%d)", capacity);
  Y3_REQUIRE(tile_rows >= 1, "y3_merge_tiled: tile_rows must be positive (%d)", tile_rows);
  Y3_REQUIRE(capacity % tile_rows == 0, "y3_merge_tiled: capacity %d is no multiple of tile_rows %d", capacity, tile_rows);
  Y3_REQUIRE(std::isfinite(thr) && thr >= 0.0 && thr <= 1.0, "y3_merge_tiled: thr must be a finite number in [0, 1] (%g)", thr);
  const WsLayout w = ws_layout(batch, capacity);
  // outputs (and the part of the workspace that is used) must not alias inputs: the inputs are read while the outputs are written
  const size_t n = (size_t)batch * (size_t)capacity;
  const struct { const char *name; const void *ptr; size_t bytes; } ins[] = {
      {"d_det_count", d_det_count, (size_t)batch * 4}, {"d_det_tlbr", d_det_tlbr, n * 32}, {"d_det_prob", d_det_prob, n * 4},
      {"d_det_cls", d_det_cls, n * 8},                 {"d_det_row", d_det_row, n * 4}},
    outs[] = {
      {"d_out_count", d_out_count, (size_t)batch * 4}, {"d_out_tlbr", d_out_tlbr, n * 32}, {"d_out_prob", d_out_prob, n * 4},
      {"d_out_cls", d_out_cls, n * 8},                 {"d_out_row", d_out_row, n * 4},
      {"d_out_members", d_out_members, d_out_members ? n * 4 : 0}, {"d_workspace", d_workspace, w.total}};
  for (const auto &o : outs)
    for (const auto &i : ins)
      Y3_REQUIRE(!o.bytes || !overlaps(o.ptr, o.bytes, i.ptr, i.bytes), "y3_merge_tiled: %s aliases %s", o.name, i.name);
  Y3_REQUIRE(workspace_bytes >= w.total, "y3_merge_tiled: workspace too small (%zu < %zu)", workspace_bytes, w.total);

  MergeArgs a = {};
  a.in_count = d_det_count; a.in_tlbr = reinterpret_cast<const long long *>(d_det_tlbr); a.in_prob = d_det_prob;
  a.in_cls = reinterpret_cast<const long long *>(d_det_cls); a.in_row = d_det_row;
  a.capacity = capacity; a.tile_rows = tile_rows; a.thr = thr;
  char *ws = static_cast<char *>(d_workspace);
  a.owner = reinterpret_cast<int *>(ws + w.owner);
  a.slot = reinterpret_cast<int *>(ws + w.slot);
  a.items = reinterpret_cast<int *>(ws + w.items);
  a.out_count = d_out_count; a.out_tlbr = reinterpret_cast<long long *>(d_out_tlbr); a.out_prob = d_out_prob;
  a.out_cls = reinterpret_cast<long long *>(d_out_cls); a.out_row = d_out_row; a.out_members = d_out_members;
  hipStream_t s = static_cast<hipStream_t>(stream);
  Y3_LAUNCH(tile_merge_kernel, dim3(batch), dim3(kThreads), 0, s, a);
  Y3_HIP_CHECK(hipGetLastError());
  return Y3_OK;
}
