// ROI geometry shared by csrc/roi_pool.hip and csrc/roi_align.hip: the ROIPooling window arithmetic (forward kernels and the ordered
// backward that re-derives the forward's bins evaluate the same bits only while they share it), the ROIAlign sample coordinate and its
// per-axis footprint / weight-sum loops, and the pyramid-level selector of both files' argument structs.
#pragma once
#include "common.h"

namespace relnet {

// Field f of pyramid level l (0..3) of an argument struct g with a `lv[4]` member.  Constant indices only: a dynamic index into the
// kernarg array forces a scratch copy of the struct (6x slower), so the helpers that use this take g by const reference and are
// force-inlined, and the kernel-argument struct itself is never written.
#define RELNET_LV_SEL4(g, l, f) ((l) == 0 ? (g).lv[0].f : (l) == 1 ? (g).lv[1].f : (l) == 2 ? (g).lv[2].f : (g).lv[3].f)

#pragma clang fp contract(off)
// ---- ROIPooling (MXNet v1.1.0 src/operator/roi_pooling.cu): the roi's integer window on a map and the cells of one bin
struct RoiWindow { int rs_h, rs_w, rh, rw; float bin_h, bin_w; };      // start cell, extent in cells (>= 1), bin size in cells
__device__ __forceinline__ RoiWindow roi_window(const float* roi, float scale, int PH, int PW) {
  RoiWindow q;
  q.rs_w = (int)roundf(roi[1] * scale); q.rs_h = (int)roundf(roi[2] * scale);
  const int re_w = (int)roundf(roi[3] * scale), re_h = (int)roundf(roi[4] * scale);
  q.rw = max(re_w - q.rs_w + 1, 1); q.rh = max(re_h - q.rs_h + 1, 1);   // malformed -> 1x1
  q.bin_h = (float)q.rh / (float)PH; q.bin_w = (float)q.rw / (float)PW;
  return q;
}
// cells [s, e) of bin p along one axis of a map of extent L (e <= s: the bin is empty)
__device__ __forceinline__ void roi_bin_span(int p, int start, float bin, int L, int& s, int& e) {
  s = min(max((int)floorf((float)p * bin) + start, 0), L);
  e = min(max((int)ceilf((float)(p + 1) * bin) + start, 0), L);
}

// ---- ROIAlign: coordinate of sample i (of `grid`) of bin p along one axis
__device__ __forceinline__ float roi_align_coord(float start, int p, float bin, int i, int grid) {
  return start + (float)p * bin + ((float)i + 0.5f) * bin / (float)grid;
}
// One axis of a roi's footprint: the cell range that the corners of every sample inside the map cover, over all P bins, folded into
// the workgroup's LDS words *lo / *hi (256 threads).
__device__ __forceinline__ void roi_align_axis_footprint(float start, float bin, int grid, int P, int L, int* lo, int* hi) {
  for (int s = threadIdx.x; s < P * grid; s += 256) {
    float y = roi_align_coord(start, s / grid, bin, s % grid, grid);
    if (y < -1.f || y > (float)L) continue;
    if (y <= 0.f) y = 0.f;
    const int yl = min((int)y, L - 1), yh = min(yl + 1, L - 1);
    atomicMin(lo, yl); atomicMax(hi, yh);
  }
}
// One axis of the patch form: w[p * stride + f] = (sum, in sample order, of the bilinear weights that the samples of bin p give cell
// c0 + f) / div, for the F cells of the footprint (256 threads).
__device__ __forceinline__ void roi_align_axis_weights(float start, float bin, int grid, int P, int L, int c0, int F, float div,
                                                       float* w, int stride) {
  for (int s = threadIdx.x; s < P * F; s += 256) {
    const int p = s / F, cell = c0 + s % F;
    float a = 0.f;
    for (int i = 0; i < grid; ++i) {
      float y = roi_align_coord(start, p, bin, i, grid);
      if (y < -1.f || y > (float)L) continue;
      if (y <= 0.f) y = 0.f;
      int yl = (int)y, yh;
      if (yl >= L - 1) { yh = yl = L - 1; y = (float)yl; } else yh = yl + 1;
      const float ly = y - (float)yl;
      if (yl == cell) a += 1.f - ly;
      if (yh == cell) a += ly;
    }
    w[p * stride + s % F] = a / div;
  }
}
#pragma clang fp contract(fast)

// Host side of the levels entry points: slot l of the four kernel-argument levels comes from entry s of the caller's num_levels (1..4)
// arrays, slots past num_levels repeat the last entry.  fill(l, s) returns 0 or an error code, which ends the walk.
template <typename F>
static inline int roi_fill_levels(int num_levels, F&& fill) {
  for (int l = 0; l < 4; ++l)
    if (const int rc = fill(l, l < num_levels ? l : num_levels - 1)) return rc;
  return 0;
}

}  // namespace relnet
