// Darknet's letterbox geometry (letterbox_image), shared by the letterbox kernel's host side (letterbox.hip) and the box
// correction of the detection tail (detect.hip), so both read ONE definition: include/yolov3_hip.h, y3_letterbox_geometry.
#pragma once

#include <stdint.h>

struct Y3LetterboxGeom {
  int new_h, new_w, top, left;
};

// h, w, net_h, net_w > 0.  float32 quotients for the choice of the side that fills the network, int64 products truncated.
__host__ __device__ inline Y3LetterboxGeom y3_letterbox_geom(int h, int w, int net_h, int net_w) {
  Y3LetterboxGeom g;
  if ((float)net_w / (float)w < (float)net_h / (float)h) {
    g.new_w = net_w;
    g.new_h = (int)((int64_t)h * net_w / w);
  } else {
    g.new_h = net_h;
    g.new_w = (int)((int64_t)w * net_h / h);
  }
  if (g.new_h < 1) g.new_h = 1;   // Darknet would make a zero-sized image
  if (g.new_w < 1) g.new_w = 1;
  g.top = (net_h - g.new_h) / 2;
  g.left = (net_w - g.new_w) / 2;
  return g;
}
