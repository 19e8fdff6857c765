// Darknet letterboxing on device (letterbox_image): every frame of a batch -- sizes may differ -- is resized with its aspect
// ratio kept, by the arithmetic of y3_resize_bilinear_u8 (layers.hip: OpenCV's 8-bit INTER_LINEAR, tap tables from the
// host), and pasted at (top, left) of a net-sized canvas of one fill byte.  Not in the reference, which stretches every frame
// (cv2.resize, inference.py:320-326); the host restatement is yolov3/preprocess.py: letterbox_u8.
//
// One launch takes up to kLbFrames frames: their descriptors are kernel arguments (no device staging buffer, nothing to keep
// alive after the call), blockIdx.y picks the frame.  A block covers 1024 output pixels, 256 per wave and 4 per lane.  A lane
// packs its 12 bytes into LDS, then 48 lanes of the wave store the wave's 768 bytes as contiguous 16-byte words (lane i at
// base + 16 i): a row of 3 * net_w bytes is no multiple of 16 per pixel, but 256 pixels are.  Pad-band pixels take the fill
// byte without loading anything.
//
// A frame without tap tables is copied 1:1 (y3_tiles_u8: a window of a larger frame cut out at full resolution): the frame's
// pixel (ty, tx) comes from src + ty * pitch + 3 * tx, where src already points at the window's first pixel and pitch is the row
// pitch of the frame the window lies in.  Same launch, same stores; the branch is uniform across a workgroup.
#include "common.h"
#include "letterbox.h"

#include <limits.h>

namespace {

constexpr int kLbFrames = 32;                      // frame descriptors per launch (48 B each: 1.5 KiB of the 4-KiB kernarg limit)
constexpr int kLbThreads = 256;
constexpr int kLbWaves = kLbThreads / 64;
constexpr int kLbLanePix = 4;                      // pixels per lane: 12 bytes = 3 dwords
constexpr int kLbWavePix = 64 * kLbLanePix;        // 256 pixels = 768 bytes = 48 16-byte words
constexpr int kLbBlockPix = kLbWaves * kLbWavePix;
constexpr int kLbMaxBlocks = 2048;                 // per launch; larger grids stride

struct LbFrame {
  const uint8_t *src;
  const int *ytab, *xtab;   // both null: the copy form, (new_h, new_w) source pixels from `src` on, 1:1
  int pitch;                // bytes from one source row to the next
  int new_h, new_w, top, left;
};

struct LbArgs {
  LbFrame f[kLbFrames];
  uint8_t *dst;     // frame 0 of this launch
  int npix;         // net_h * net_w
  int net_w;
  int fill;
  int vec;          // dst and 3 * npix are multiples of 16: 16-byte stores
};

__global__ __launch_bounds__(kLbThreads) void letterbox_u8_kernel(LbArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t stage[kLbWaves][kLbWavePix * 3 / 4];
  const LbFrame &fr = a.f[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nbytes = a.npix * 3;
  uint8_t *dst = a.dst + (long long)blockIdx.y * nbytes;
  const int y_end = fr.top + fr.new_h, x_end = fr.left + fr.new_w;
  const uint8_t fill = (uint8_t)a.fill;
  // the trip count is the same for every wave of the block (barriers below); a wave past the frame's end stores nothing
  for (int base = blockIdx.x * kLbBlockPix; base < a.npix; base += gridDim.x * kLbBlockPix) {
    const int wbase = base + wave * kLbWavePix;
    const int p0 = wbase + lane * kLbLanePix;
    uint8_t px[kLbLanePix * 3];
    int y = p0 / a.net_w, x = p0 - y * a.net_w;
#pragma unroll
    for (int k = 0; k < kLbLanePix; ++k) {
      const bool inside = p0 + k < a.npix && y >= fr.top && y < y_end && x >= fr.left && x < x_end;
      const int ty = y - fr.top, tx = x - fr.left;
      if (inside && !fr.ytab) {
        const uint8_t *s = fr.src + (long long)ty * fr.pitch + tx * 3;
        px[k * 3 + 0] = s[0]; px[k * 3 + 1] = s[1]; px[k * 3 + 2] = s[2];
      } else if (inside) {
        const int ylo = fr.ytab[ty * 4 + 0], yhi = fr.ytab[ty * 4 + 1], wy0 = fr.ytab[ty * 4 + 2], wy1 = fr.ytab[ty * 4 + 3];
        const int xlo = fr.xtab[tx * 4 + 0], xhi = fr.xtab[tx * 4 + 1], wx0 = fr.xtab[tx * 4 + 2], wx1 = fr.xtab[tx * 4 + 3];
        const uint8_t *r0 = fr.src + (long long)ylo * fr.pitch, *r1 = fr.src + (long long)yhi * fr.pitch;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          // y3_resize_bilinear_u8's two truncating stages (layers.hip: resize_u8_kernel)
          const int top = r0[xlo * 3 + c] * wx0 + r0[xhi * 3 + c] * wx1;
          const int bot = r1[xlo * 3 + c] * wx0 + r1[xhi * 3 + c] * wx1;
          int v = (((wy0 * (top >> 4)) >> 16) + ((wy1 * (bot >> 4)) >> 16) + 2) >> 2;
          v = v < 0 ? 0 : (v > 255 ? 255 : v);
          px[k * 3 + c] = (uint8_t)v;
        }
      } else {
        px[k * 3 + 0] = px[k * 3 + 1] = px[k * 3 + 2] = fill;
      }
      if (++x == a.net_w) { x = 0; ++y; }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
      stage[wave][lane * 3 + i] = (uint32_t)px[4 * i] | ((uint32_t)px[4 * i + 1] << 8) | ((uint32_t)px[4 * i + 2] << 16) |
                                  ((uint32_t)px[4 * i + 3] << 24);
    __syncthreads();
    if (lane < kLbWavePix * 3 / 16) {
      const int off = wbase * 3 + lane * 16;           // byte offset in the frame
      if (a.vec && off + 16 <= nbytes) {
        *reinterpret_cast<u32x4 *>(dst + off) = *reinterpret_cast<const u32x4 *>(&stage[wave][lane * 4]);
      } else {
        const uint8_t *sb = reinterpret_cast<const uint8_t *>(&stage[wave][lane * 4]);
        for (int j = 0; j < 16 && off + j < nbytes; ++j) dst[off + j] = sb[j];
      }
    }
    __syncthreads();   // stage is rewritten by the next tile
  }
}

}  // namespace

extern "C" int y3_letterbox_geometry(int src_h, int src_w, int net_h, int net_w, int32_t out[4]) {
  Y3_REQUIRE(out, "y3_letterbox_geometry: null pointer argument");
  Y3_REQUIRE(src_h > 0 && src_w > 0 && net_h > 0 && net_w > 0, "y3_letterbox_geometry: sizes must be positive");
  const Y3LetterboxGeom g = y3_letterbox_geom(src_h, src_w, net_h, net_w);
  out[0] = g.new_h; out[1] = g.new_w; out[2] = g.top; out[3] = g.left;
  return Y3_OK;
}

namespace {
// what y3_letterbox_u8 and y3_tiles_u8 share: the checks of the canvas, and `count` frames in launches of kLbFrames, frame i
// described by frame(i)
template <typename FRAME>
int lb_launch(const char *who, int count, uint8_t *d_dst, int net_h, int net_w, int fill, void *stream, FRAME frame) {
  Y3_REQUIRE(count > 0 && net_h > 0 && net_w > 0, "%s: batch and network size must be positive", who);
  Y3_REQUIRE(((long long)net_h * net_w + kLbBlockPix) * 3 <= INT_MAX, "%s: network size %d x %d too large", who, net_h, net_w);
  Y3_REQUIRE(fill >= 0 && fill <= 255, "%s: fill %d is not a byte", who, fill);
  LbArgs a = {};
  a.npix = net_h * net_w;
  a.net_w = net_w;
  a.fill = fill;
  const size_t nbytes = (size_t)a.npix * 3;
  a.vec = ((uintptr_t)d_dst & 15) == 0 && nbytes % 16 == 0;
  const int tiles = (a.npix + kLbBlockPix - 1) / kLbBlockPix;
  for (int b0 = 0; b0 < count; b0 += kLbFrames) {
    const int n = count - b0 < kLbFrames ? count - b0 : kLbFrames;
    for (int i = 0; i < n; ++i) a.f[i] = frame(b0 + i);
    a.dst = d_dst + (size_t)b0 * nbytes;
    const int bx = tiles < kLbMaxBlocks / n ? tiles : (kLbMaxBlocks / n > 0 ? kLbMaxBlocks / n : 1);
    Y3_LAUNCH(letterbox_u8_kernel, dim3(bx, n), dim3(kLbThreads), 0, static_cast<hipStream_t>(stream), a);
    Y3_HIP_CHECK(hipGetLastError());
  }
  return Y3_OK;
}
}  // namespace

extern "C" int y3_letterbox_u8(const y3_letterbox_frame *frames, int batch, uint8_t *d_dst, int net_h, int net_w, int fill,
                               void *stream) {
  Y3_REQUIRE(frames && d_dst, "y3_letterbox_u8: null pointer argument");
  for (int i = 0; i < batch; ++i) {
    Y3_REQUIRE(frames[i].d_src && frames[i].d_ytab && frames[i].d_xtab && frames[i].src_h > 0 && frames[i].src_w > 0,
               "y3_letterbox_u8: frame %d: null pointer or empty frame", i);
    Y3_REQUIRE(frames[i].src_w <= INT_MAX / 3, "y3_letterbox_u8: frame %d: %d columns are too many", i, frames[i].src_w);
  }
  return lb_launch("y3_letterbox_u8", batch, d_dst, net_h, net_w, fill, stream, [&](int i) {
    const y3_letterbox_frame &f = frames[i];
    const Y3LetterboxGeom g = y3_letterbox_geom(f.src_h, f.src_w, net_h, net_w);
    return LbFrame{f.d_src, f.d_ytab, f.d_xtab, f.src_w * 3, g.new_h, g.new_w, g.top, g.left};
  });
}

extern "C" int y3_tiles_u8(const y3_tile *tiles, int n_tiles, uint8_t *d_dst, int net_h, int net_w, int fill, void *stream) {
  Y3_REQUIRE(tiles && d_dst, "y3_tiles_u8: null pointer argument");
  for (int i = 0; i < n_tiles; ++i) {
    const y3_tile &t = tiles[i];
    Y3_REQUIRE(t.d_src && t.src_h > 0 && t.src_w > 0, "y3_tiles_u8: tile %d: null pointer or empty frame", i);
    Y3_REQUIRE(t.src_w <= INT_MAX / 3, "y3_tiles_u8: tile %d: %d columns are too many", i, t.src_w);
    Y3_REQUIRE(t.y0 >= 0 && t.y0 < t.src_h && t.x0 >= 0 && t.x0 < t.src_w,
               "y3_tiles_u8: tile %d: origin (%d, %d) lies outside its %d x %d frame", i, t.y0, t.x0, t.src_h, t.src_w);
  }
  return lb_launch("y3_tiles_u8", n_tiles, d_dst, net_h, net_w, fill, stream, [&](int i) {
    const y3_tile &t = tiles[i];
    const int h = t.src_h - t.y0 < net_h ? t.src_h - t.y0 : net_h, w = t.src_w - t.x0 < net_w ? t.src_w - t.x0 : net_w;
    return LbFrame{t.d_src + ((size_t)t.y0 * t.src_w + t.x0) * 3, nullptr, nullptr, t.src_w * 3, h, w, 0, 0};
  });
}
