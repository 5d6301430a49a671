// JPEG ingest: the plane geometry shared by the host planner (jpeg_host.cpp) and the device
// kernels (jpeg.hip), and the device-readable descriptor blob of a batch
// (rtdm_jpeg_batch_plan writes it, the two batch kernels read it).
#pragma once

#include <algorithm>

#include "common.h"

namespace rtdm {

struct JpegPlanes {
  int ncomp, w, h;
  int bw[3], bh[3];   // block grids
  int64_t off[3];     // first block of each component in the coefficient buffer
  int64_t poff[3];    // byte offset of each component's sample plane (pitch bw * 8)
  int h_samp[3], v_samp[3], hmax, vmax;
};

inline JpegPlanes planes_of(const rtdm_jpeg_info& in, int64_t* bytes) {
  JpegPlanes p{};
  p.ncomp = in.ncomp;
  p.w = in.width;
  p.h = in.height;
  p.hmax = p.vmax = 1;
  int64_t o = 0;
  for (int c = 0; c < in.ncomp; ++c) {
    p.bw[c] = in.bw[c];
    p.bh[c] = in.bh[c];
    p.off[c] = in.coef_off[c];
    p.h_samp[c] = in.h[c];
    p.v_samp[c] = in.v[c];
    p.hmax = std::max(p.hmax, in.h[c]);
    p.vmax = std::max(p.vmax, in.v[c]);
    p.poff[c] = o;
    o += (int64_t)in.bw[c] * 8 * in.bh[c] * 8;
  }
  if (bytes) *bytes = o;
  return p;
}

// The sampling layouts the reconstruct kernels handle: grayscale, or three components with
// 1x1 chroma and 1x1 / 2x1 / 2x2 luma.  Returns the colour kernel's mode, -1 if refused.
enum JpegMode : int { JPEG_GRAY = 0, JPEG_444 = 1, JPEG_H2V1 = 2, JPEG_H2V2 = 3 };
inline int jpeg_mode(int ncomp, const int* h, const int* v) {
  if (ncomp == 1) return JPEG_GRAY;
  if (ncomp != 3 || h[1] != 1 || v[1] != 1 || h[2] != 1 || v[2] != 1) return -1;
  if (h[0] == 1 && v[0] == 1) return JPEG_444;
  if (h[0] == 2 && v[0] == 1) return JPEG_H2V1;
  if (h[0] == 2 && v[0] == 2) return JPEG_H2V2;
  return -1;
}

// Batch kernels' workgroup shapes: one thread per 8x8 block; one thread per kJpegColorPx
// horizontally adjacent output pixels.
constexpr int kJpegIdctWG = 256;
constexpr int kJpegColorWG = 256;
constexpr int kJpegColorPx = 4;

// Descriptor blob: JpegBatchHead, then one JpegBatchImage per image of the batch (index
// order; a refused image has no workgroups).  Workgroup g of a launch belongs to the last
// image whose first workgroup (idct_wg0 / color_wg0, prefix sums) is <= g.
struct JpegBatchHead {
  int32_t n, idct_groups, color_groups;
  int32_t pad[13];
};
struct JpegBatchImage {
  JpegPlanes p;        // off[]: blocks from the arena start; poff[]: bytes from the workspace start
  int64_t nblocks;     // blocks of the image: arena [p.off[0], p.off[0] + nblocks)
  int64_t out_off, out_pitch;
  int32_t idct_wg0, color_wg0;
  int32_t qt_slot;
  int32_t mode;        // JpegMode
  int32_t flat;        // out_pitch == 3 * w: the image's pixels are one contiguous run
  int32_t skip;        // entropy decode failed: the kernels leave the image alone
  int32_t cw, ch;      // chroma plane size (downsampled)
  int32_t pad[4];
};
static_assert(sizeof(JpegBatchHead) == 64 && sizeof(JpegBatchImage) == 192, "RTDM_JPEG_BATCH_DESC_BYTES");

}  // namespace rtdm
