// Darknet's own preprocessing on device: uint8 BGR frames of any size -> the float32 planar RGB network input that Darknet's
// load_image -> letterbox_image / resize_image produce, bit for bit.  Not in the reference, which resizes 8-bit frames with
// cv2.resize; include/yolov3_hip.h (y3_preprocess_darknet_f32) states every operation, tests/darknet_resize_restate.py restates
// it in numpy as the two-pass form with an explicit `part` image.
//
// This file is compiled with -ffp-contract=off (csrc/Makefile: STRICT): every product and sum below rounds on its own, as
// Darknet's separately stored floats do.  An output value needs at most four source pixels: the horizontal blend of its two
// source rows (`part` values, plain float32 either way) and their vertical blend, all in registers -- no tap tables, no
// intermediate image.
//
// One launch takes up to kDkFrames frames: their descriptors are kernel arguments (nothing to stage or keep alive),
// blockIdx.y picks the frame.  A lane computes four consecutive pixels of a row for all three channels -- the three bytes of a
// source pixel are neighbours -- and stores one 16-byte word per plane, so a wave writes 1 KiB of consecutive addresses per
// plane and store.  A network width that is no multiple of 4 (or an unaligned destination) takes 4-byte stores.  byte / 255 comes from a
// 256-entry table (one IEEE division per entry and workgroup, as in conv_small.hip); pad pixels load nothing.
#include "common.h"
#include "letterbox.h"

#include <limits.h>

namespace {

constexpr int kDkFrames = 64;                      // frame descriptors per launch (40 B each: 2.5 KiB of the 4-KiB kernarg limit)
constexpr int kDkThreads = 256;
constexpr int kDkLanePix = 4;                      // pixels per lane: one 16-byte store per plane
constexpr int kDkBlockPix = kDkThreads * kDkLanePix;
constexpr int kDkMaxBlocks = 2048;                 // per launch; larger grids stride
constexpr int kDkMaxDim = 1 << 24;                 // every row / column index is exact in float32

struct DkFrame {
  const uint8_t *src;
  int src_h, src_w, new_h, new_w, top, left;
  float h_scale, w_scale;                          // (float)(src - 1) / (float)(new - 1); 0 where the axis has one source pixel
};

struct DkArgs {
  DkFrame f[kDkFrames];
  float *dst;       // frame 0 of this launch
  int npix;         // net_h * net_w
  int net_w;
  int vec;          // dst is 16-byte aligned and net_w a multiple of 4: 16-byte stores
};

// part[r][tx] of one channel: resize_image's horizontal pass (`row` = source row r, `ch` = the byte of the BGR pixel)
__device__ __forceinline__ float dk_part(const uint8_t *row, const float *lut, int ch, bool last_col, int ix, int ix1, float dx) {
  if (last_col) return lut[row[ix1 * 3 + ch]];
  return (1.0f - dx) * lut[row[ix * 3 + ch]] + dx * lut[row[ix1 * 3 + ch]];
}

__global__ __launch_bounds__(kDkThreads) void preprocess_darknet_kernel(DkArgs a) {
  __shared__ float lut[256];                       // lut[v] = (float)v / 255.0f (== (float)(v / 255.) for every byte)
  lut[threadIdx.x] = (float)threadIdx.x / 255.0f;
  __syncthreads();
  const DkFrame &fr = a.f[blockIdx.y];
  float *dst = a.dst + (size_t)blockIdx.y * 3 * a.npix;
  const int y_end = fr.top + fr.new_h, x_end = fr.left + fr.new_w;
  const bool same = fr.new_h == fr.src_h && fr.new_w == fr.src_w;       // resize_image copies
  const size_t pitch = (size_t)fr.src_w * 3;
  for (int p0 = (blockIdx.x * kDkThreads + threadIdx.x) * kDkLanePix; p0 < a.npix; p0 += gridDim.x * kDkBlockPix) {
    float v[3][kDkLanePix];
    int y = p0 / a.net_w, x = p0 - y * a.net_w;
#pragma unroll
    for (int k = 0; k < kDkLanePix; ++k) {
      if (p0 + k < a.npix && y >= fr.top && y < y_end && x >= fr.left && x < x_end) {
        const int ty = y - fr.top, tx = x - fr.left;
        if (same) {
          const uint8_t *px = fr.src + ty * pitch + (size_t)tx * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c][k] = lut[px[2 - c]];
        } else {
          // columns: the last one (and every one of a 1-pixel-wide source) is the source's last column
          const bool last_col = tx == fr.new_w - 1 || fr.src_w == 1;
          const float sx = (float)tx * fr.w_scale;
          int ix = (int)sx;
          const float dx = sx - (float)ix;
          ix = ix < fr.src_w - 1 ? ix : fr.src_w - 1;                   // (never taken for sizes below kDkMaxDim: memory safety only)
          const int ix1 = last_col ? fr.src_w - 1 : (ix + 1 < fr.src_w - 1 ? ix + 1 : fr.src_w - 1);
          // rows: dy is NOT forced to 0 on the last row, whose second term is dropped (Darknet's quirk, kept)
          const bool last_row = ty == fr.new_h - 1 || fr.src_h == 1;
          const float sy = (float)ty * fr.h_scale;
          int iy = (int)sy;
          const float dy = sy - (float)iy;
          iy = iy < fr.src_h - 1 ? iy : fr.src_h - 1;
          const int iy1 = iy + 1 < fr.src_h - 1 ? iy + 1 : fr.src_h - 1;
          const uint8_t *r0 = fr.src + iy * pitch, *r1 = fr.src + iy1 * pitch;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float o = (1.0f - dy) * dk_part(r0, lut, 2 - c, last_col, ix, ix1, dx);
            if (!last_row) o = o + dy * dk_part(r1, lut, 2 - c, last_col, ix, ix1, dx);
            v[c][k] = o;
          }
        }
      } else {
        v[0][k] = v[1][k] = v[2][k] = 0.5f;
      }
      if (++x == a.net_w) { x = 0; ++y; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float *o = dst + (size_t)c * a.npix + p0;
      if (a.vec) {                                 // net_w % 4 == 0: the four pixels exist and lie in one row
        *reinterpret_cast<f32x4 *>(o) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
      } else {
#pragma unroll
        for (int k = 0; k < kDkLanePix; ++k)
          if (p0 + k < a.npix) o[k] = v[c][k];
      }
    }
  }
}

// (float)(src - 1) / (float)(dst - 1); an axis with one source pixel never uses its scale for an index that matters (Darknet
// computes 0 / 0 for 1 -> 1 and then reads pixel 0 with weight 1): 0 keeps every intermediate finite
float dk_scale(int src, int dst) { return src == 1 ? 0.0f : (float)(src - 1) / (float)(dst - 1); }

}  // namespace

extern "C" int y3_preprocess_darknet_f32(const y3_darknet_frame *frames, int batch, float *d_dst, int net_h, int net_w,
                                         int letterbox, void *stream) {
  Y3_REQUIRE(frames && d_dst, "y3_preprocess_darknet_f32: null pointer argument");
  Y3_REQUIRE(batch > 0 && net_h > 0 && net_w > 0, "y3_preprocess_darknet_f32: batch and network size must be positive");
  Y3_REQUIRE(net_h < kDkMaxDim && net_w < kDkMaxDim && (long long)net_h * net_w + (long long)kDkMaxBlocks * kDkBlockPix <= INT_MAX,
             "y3_preprocess_darknet_f32: network size %d x %d too large", net_h, net_w);
  Y3_REQUIRE(((uintptr_t)d_dst & 3) == 0, "y3_preprocess_darknet_f32: d_dst is not 4-byte aligned");
  for (int i = 0; i < batch; ++i) {
    const y3_darknet_frame &f = frames[i];
    Y3_REQUIRE(f.d_src && f.src_h > 0 && f.src_w > 0, "y3_preprocess_darknet_f32: frame %d: null pointer or empty frame", i);
    Y3_REQUIRE(f.src_h < kDkMaxDim && f.src_w < kDkMaxDim, "y3_preprocess_darknet_f32: frame %d: %d x %d too large", i, f.src_h,
               f.src_w);
    Y3LetterboxGeom g = {net_h, net_w, 0, 0};
    if (letterbox) g = y3_letterbox_geom(f.src_h, f.src_w, net_h, net_w);
    // Darknet divides by (target - 1): a 1-pixel target of a longer source is a division by zero there
    Y3_REQUIRE((g.new_h > 1 || f.src_h == 1) && (g.new_w > 1 || f.src_w == 1),
               "y3_preprocess_darknet_f32: frame %d: %d x %d would be resized to %d x %d (Darknet's resize_image divides by "
               "target - 1: a 1-pixel target needs a 1-pixel source)", i, f.src_h, f.src_w, g.new_h, g.new_w);
  }
  DkArgs a = {};
  a.npix = net_h * net_w;
  a.net_w = net_w;
  a.vec = ((uintptr_t)d_dst & 15) == 0 && net_w % kDkLanePix == 0;
  const int tiles = (a.npix + kDkBlockPix - 1) / kDkBlockPix;
  for (int b0 = 0; b0 < batch; b0 += kDkFrames) {
    const int n = batch - b0 < kDkFrames ? batch - b0 : kDkFrames;
    for (int i = 0; i < n; ++i) {
      const y3_darknet_frame &f = frames[b0 + i];
      Y3LetterboxGeom g = {net_h, net_w, 0, 0};
      if (letterbox) g = y3_letterbox_geom(f.src_h, f.src_w, net_h, net_w);
      a.f[i] = DkFrame{f.d_src, f.src_h, f.src_w, g.new_h, g.new_w, g.top, g.left, dk_scale(f.src_h, g.new_h),
                       dk_scale(f.src_w, g.new_w)};
    }
    a.dst = d_dst + (size_t)b0 * 3 * a.npix;
    const int bx = tiles < kDkMaxBlocks / n ? tiles : kDkMaxBlocks / n;
    Y3_LAUNCH(preprocess_darknet_kernel, dim3(bx, n), dim3(kDkThreads), 0, static_cast<hipStream_t>(stream), a);
    Y3_HIP_CHECK(hipGetLastError());
  }
  return Y3_OK;
}
