// ROIAlign forward / backward (named by BASELINE.json's north_star next to the proposal op; the reference graphs themselves pool with
// mx.symbol.ROIPooling -- symbols/resnet_v1_101_rcnn_attention_1024_pairwise_position_multi_head_16.py:252-253 -- and ship no ROIAlign, so
// this operator follows the PUBLISHED algorithm: He et al., "Mask R-CNN" (2017) section 3 as implemented by Detectron's RoIAlign /
// mx.contrib.sym.ROIAlign of MXNet >= 1.3: no coordinate rounding, sampling_ratio x sampling_ratio bilinear samples per bin, averaged).
//
//   roi_start = x1 * scale - off, roi_end = x2 * scale - off            (off = 0.5 when `aligned`, else 0)
//   roi_w = roi_end_w - roi_start_w (not aligned: max(., 1)), bin_w = roi_w / PW, grid_w = sampling_ratio > 0 ? sampling_ratio : ceil(roi_w / PW)
//   sample (iy, ix) of bin (ph, pw): y = roi_start_h + ph bin_h + (iy + 0.5) bin_h / grid_h,  x likewise
//   bilinear(y, x): 0 outside (-1, H) x (-1, W); coordinates clamped to [0, H - 1] x [0, W - 1]; out = sum / max(grid_h grid_w, 1)
//
// Explicit element strides like csrc/roi_pool.hip: NCHW fp32 (parity tests) and channels-last bf16 (thread = (bin, 8 channels), four 16-byte
// corner loads per sample).  Arithmetic in fp32 with contraction off, in the order oracle/roi_align.py restates: bit-identical on fp32 data.
#include "common.h"
#include "roi.h"

namespace relnet {

struct RoiAlignArgs {
  const void* data; long ds_b, ds_c, ds_h, ds_w;     // element strides of [B, C, H, W]
  const float* rois;                                  // [R, 5] batch_idx, x1, y1, x2, y2
  void* out; long os_r, os_c, os_ph, os_pw;           // element strides of [R, C, PH, PW]  (backward: the output GRADIENT)
  float* grad_in; long gs_b, gs_c, gs_h, gs_w;        // backward: fp32 accumulation buffer (pre-zeroed), any layout
  int R, C, H, W, PH, PW, sampling_ratio, aligned, batch_index_base;
  float scale;
  // forward kernels and the levels backward: roi r reads lv[level[r]] (level == nullptr: lv[0]).  A row whose batch index lies outside
  // [0, B) or whose level lies outside [0, num_levels) pools to zeros and contributes no gradient.
  const int* level; int num_levels, B;
  struct Level { const void* data; long ds_b, ds_c, ds_h, ds_w; float* grad; long gs_b, gs_c, gs_h, gs_w; int H, W; float scale; } lv[4];
};

#pragma clang fp contract(off)
struct RoiBin { int b; float start_h, start_w, bin_h, bin_w; int grid_h, grid_w; float count; };

__device__ __forceinline__ RoiBin roi_bin(const RoiAlignArgs& g, int r, float scale) {
  const float* roi = g.rois + (long)r * 5;
  RoiBin q;
  q.b = (int)roi[0] - g.batch_index_base;
  const float off = g.aligned ? 0.5f : 0.f;
  q.start_w = roi[1] * scale - off; q.start_h = roi[2] * scale - off;
  const float end_w = roi[3] * scale - off, end_h = roi[4] * scale - off;
  float rw = end_w - q.start_w, rh = end_h - q.start_h;
  if (!g.aligned) { rw = fmaxf(rw, 1.f); rh = fmaxf(rh, 1.f); }
  q.bin_h = rh / (float)g.PH; q.bin_w = rw / (float)g.PW;
  q.grid_h = g.sampling_ratio > 0 ? g.sampling_ratio : (int)ceilf(rh / (float)g.PH);
  q.grid_w = g.sampling_ratio > 0 ? g.sampling_ratio : (int)ceilf(rw / (float)g.PW);
  q.count = fmaxf((float)(q.grid_h * q.grid_w), 1.f);
  return q;
}

// The map of roi r as plain scalars (RELNET_LV_SEL4: constant indices only).  ok == false: invalid batch index or level -> the caller
// writes zeros / adds nothing (the fields then describe level 0 and are not dereferenced).
struct RoiAlignMap { const void* data; long ds_b, ds_c, ds_h, ds_w; float* grad; long gs_b, gs_c, gs_h, gs_w; int H, W; float scale; bool ok; };
__device__ __forceinline__ RoiAlignMap roi_align_map(const RoiAlignArgs& g, int r) {
  RoiAlignMap m;
  int l = g.level ? g.level[r] : 0;
  const int b = (int)g.rois[(long)r * 5] - g.batch_index_base;
  m.ok = l >= 0 && l < g.num_levels && b >= 0 && b < g.B;
  if (!m.ok) l = 0;
#define LV(f) RELNET_LV_SEL4(g, l, f)
  m.data = LV(data); m.ds_b = LV(ds_b); m.ds_c = LV(ds_c); m.ds_h = LV(ds_h); m.ds_w = LV(ds_w);
  m.grad = LV(grad); m.gs_b = LV(gs_b); m.gs_c = LV(gs_c); m.gs_h = LV(gs_h); m.gs_w = LV(gs_w);
  m.H = LV(H); m.W = LV(W); m.scale = LV(scale);
#undef LV
  return m;
}

// the four corners and weights of one sample; returns false when the sample lies outside the map (contributes 0)
struct Corners { int yl, xl, yh, xh; float w1, w2, w3, w4; };
__device__ __forceinline__ bool corners(float y, float x, int H, int W, Corners& c) {
  if (y < -1.f || y > (float)H || x < -1.f || x > (float)W) return false;
  if (y <= 0.f) y = 0.f;
  if (x <= 0.f) x = 0.f;
  c.yl = (int)y; c.xl = (int)x;
  if (c.yl >= H - 1) { c.yh = c.yl = H - 1; y = (float)c.yl; } else c.yh = c.yl + 1;
  if (c.xl >= W - 1) { c.xh = c.xl = W - 1; x = (float)c.xl; } else c.xh = c.xl + 1;
  const float ly = y - (float)c.yl, lx = x - (float)c.xl, hy = 1.f - ly, hx = 1.f - lx;
  c.w1 = hy * hx; c.w2 = hy * lx; c.w3 = ly * hx; c.w4 = ly * lx;
  return true;
}

// grid.x = R * PH * PW bins, threads stride over channels (any layout)
template <typename T>
__global__ __launch_bounds__(256) void roi_align_fwd_kernel(RoiAlignArgs g) {
  const int bin = blockIdx.x;
  const int pw = bin % g.PW, ph = (bin / g.PW) % g.PH, r = bin / (g.PW * g.PH);
  const RoiAlignMap m = roi_align_map(g, r);
  T* out = (T*)g.out + (long)r * g.os_r + (long)ph * g.os_ph + (long)pw * g.os_pw;
  if (!m.ok) {
    for (int c = threadIdx.x; c < g.C; c += 256) stf<T>(out + (long)c * g.os_c, 0.f);
    return;
  }
  const RoiBin q = roi_bin(g, r, m.scale);
  const T* base = (const T*)m.data + (long)q.b * m.ds_b;
  for (int c = threadIdx.x; c < g.C; c += 256) {
    const T* pc = base + (long)c * m.ds_c;
    float sum = 0.f;
    for (int iy = 0; iy < q.grid_h; ++iy) {
      const float y = roi_align_coord(q.start_h, ph, q.bin_h, iy, q.grid_h);
      for (int ix = 0; ix < q.grid_w; ++ix) {
        const float x = roi_align_coord(q.start_w, pw, q.bin_w, ix, q.grid_w);
        Corners k;
        if (!corners(y, x, m.H, m.W, k)) continue;
        const float v1 = ldf<T>(pc + (long)k.yl * m.ds_h + (long)k.xl * m.ds_w), v2 = ldf<T>(pc + (long)k.yl * m.ds_h + (long)k.xh * m.ds_w);
        const float v3 = ldf<T>(pc + (long)k.yh * m.ds_h + (long)k.xl * m.ds_w), v4 = ldf<T>(pc + (long)k.yh * m.ds_h + (long)k.xh * m.ds_w);
        sum += ((k.w1 * v1 + k.w2 * v2) + k.w3 * v3) + k.w4 * v4;
      }
    }
    stf<T>(out + (long)c * g.os_c, sum / q.count);
  }
}

// Channels-last bf16: thread = (bin, 8-channel group); a sample = four 16-byte corner loads.  C % 8 == 0, ds_c == os_c == 1.
// grid.x = R * blocks_per_roi (R folded into x: no 65 535 limit on the roi count).
__global__ __launch_bounds__(256) void roi_align_fwd_cl_kernel(RoiAlignArgs g, int blocks_per_roi) {
  const int groups = g.C >> 3;
  const int bins_per_blk = 256 / groups;
  const int r = blockIdx.x / blocks_per_roi;
  const int bin = (blockIdx.x % blocks_per_roi) * bins_per_blk + threadIdx.x / groups;
  const int cg = threadIdx.x % groups;
  if (bin >= g.PH * g.PW) return;
  const int pw = bin % g.PW, ph = bin / g.PW;
  const RoiAlignMap m = roi_align_map(g, r);
  float sum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sum[e] = 0.f;
  if (m.ok) {
    const RoiBin q = roi_bin(g, r, m.scale);
    const unsigned short* base = (const unsigned short*)m.data + (long)q.b * m.ds_b + cg * 8;
    for (int iy = 0; iy < q.grid_h; ++iy) {
      const float y = roi_align_coord(q.start_h, ph, q.bin_h, iy, q.grid_h);
      for (int ix = 0; ix < q.grid_w; ++ix) {
        const float x = roi_align_coord(q.start_w, pw, q.bin_w, ix, q.grid_w);
        Corners k;
        if (!corners(y, x, m.H, m.W, k)) continue;
        const uint4 a1 = *(const uint4*)(base + (long)k.yl * m.ds_h + (long)k.xl * m.ds_w), a2 = *(const uint4*)(base + (long)k.yl * m.ds_h + (long)k.xh * m.ds_w);
        const uint4 a3 = *(const uint4*)(base + (long)k.yh * m.ds_h + (long)k.xl * m.ds_w), a4 = *(const uint4*)(base + (long)k.yh * m.ds_h + (long)k.xh * m.ds_w);
        const unsigned int u1[4] = {a1.x, a1.y, a1.z, a1.w}, u2[4] = {a2.x, a2.y, a2.z, a2.w}, u3[4] = {a3.x, a3.y, a3.z, a3.w}, u4[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sum[2 * e] += ((k.w1 * bf2f(u1[e] & 0xffff) + k.w2 * bf2f(u2[e] & 0xffff)) + k.w3 * bf2f(u3[e] & 0xffff)) + k.w4 * bf2f(u4[e] & 0xffff);
          sum[2 * e + 1] += ((k.w1 * bf2f(u1[e] >> 16) + k.w2 * bf2f(u2[e] >> 16)) + k.w3 * bf2f(u3[e] >> 16)) + k.w4 * bf2f(u4[e] >> 16);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] = sum[e] / q.count;
  }
  const long o = (long)r * g.os_r + (long)ph * g.os_ph + (long)pw * g.os_pw + cg * 8;
  *(uint4*)((unsigned short*)g.out + o) = make_uint4(pack_bf16x2(sum[0], sum[1]), pack_bf16x2(sum[2], sum[3]),
                                                     pack_bf16x2(sum[4], sum[5]), pack_bf16x2(sum[6], sum[7]));
}

// Backward: every sample scatters w_k * dOut / count to its four corners (fp32 atomics; with a channels-last accumulation buffer the lanes'
// consecutive channels hit consecutive words).  grid.x = R * PH * PW bins, threads stride over channels.
template <typename T>
__global__ __launch_bounds__(256) void roi_align_bwd_kernel(RoiAlignArgs g) {
  const int bin = blockIdx.x;
  const int pw = bin % g.PW, ph = (bin / g.PW) % g.PH, r = bin / (g.PW * g.PH);
  const RoiBin q = roi_bin(g, r, g.scale);
  float* gb = g.grad_in + (long)q.b * g.gs_b;
  for (int c = threadIdx.x; c < g.C; c += 256) {
    const float go = ldf<T>((const T*)g.out + (long)r * g.os_r + (long)c * g.os_c + (long)ph * g.os_ph + (long)pw * g.os_pw) / q.count;
    float* gc = gb + (long)c * g.gs_c;
    for (int iy = 0; iy < q.grid_h; ++iy) {
      const float y = roi_align_coord(q.start_h, ph, q.bin_h, iy, q.grid_h);
      for (int ix = 0; ix < q.grid_w; ++ix) {
        const float x = roi_align_coord(q.start_w, pw, q.bin_w, ix, q.grid_w);
        Corners k;
        if (!corners(y, x, g.H, g.W, k)) continue;
        atomicAdd(gc + (long)k.yl * g.gs_h + (long)k.xl * g.gs_w, k.w1 * go);
        atomicAdd(gc + (long)k.yl * g.gs_h + (long)k.xh * g.gs_w, k.w2 * go);
        atomicAdd(gc + (long)k.yh * g.gs_h + (long)k.xl * g.gs_w, k.w3 * go);
        atomicAdd(gc + (long)k.yh * g.gs_h + (long)k.xh * g.gs_w, k.w4 * go);
      }
    }
  }
}

// Backward of the levels entry: one workgroup per roi, threads over channels.  The sample weights of a bin factor into a row weight times
// a column weight -- bilinear weights, clamping, the out-of-map test (y and x are tested separately) and 1/count alike -- so the roi's
// whole contribution to one channel is the patch Wy^T Go Wx over its footprint of FH x FW cells, where Go is the PH x PW output gradient
// and Wy [PH][FH] / Wx [PW][FW] hold per-axis weight sums (LDS, shared by all channels).  The patch is added with one float atomic per
// (cell, channel), lanes over consecutive channels (NHWC: 256 contiguous bytes per wave instruction): a 10 x 10-cell roi issues 121
// adds per channel where the per-sample scatter issues 7 x 7 x 2 x 2 x 4 = 784.  A roi whose footprint exceeds RA_PATCH_MAX cells per
// axis, or whose patch has more cells than the scatter has adds, keeps the per-sample scatter (same workgroup, any pooled size).
#define RA_PATCH_MAX 64
template <typename T, int P>          // P = 7: PH == PW == 7 (the patch form); P = 0: any pooled size, scatter only
__global__ __launch_bounds__(256) void roi_align_bwd_levels_kernel(RoiAlignArgs g) {
  __shared__ float s_wy[(P ? P : 1) * RA_PATCH_MAX], s_wx[(P ? P : 1) * RA_PATCH_MAX];
  __shared__ int s_lo[2], s_hi[2];
  const int r = blockIdx.x;
  const RoiAlignMap m = roi_align_map(g, r);
  if (!m.ok) return;
  const RoiBin q = roi_bin(g, r, m.scale);
  float* gb = m.grad + (long)q.b * m.gs_b;
  const T* go_r = (const T*)g.out + (long)r * g.os_r;
  if (P) {
    constexpr int PP = P ? P : 1;
    // footprint: the cell range every valid sample's corners cover, per axis
    if (threadIdx.x < 2) { s_lo[threadIdx.x] = INT_MAX; s_hi[threadIdx.x] = -1; }
    __syncthreads();
    roi_align_axis_footprint(q.start_h, q.bin_h, q.grid_h, PP, m.H, &s_lo[0], &s_hi[0]);
    roi_align_axis_footprint(q.start_w, q.bin_w, q.grid_w, PP, m.W, &s_lo[1], &s_hi[1]);
    __syncthreads();
    const int y0 = s_lo[0], x0 = s_lo[1];
    const int FH = s_hi[0] - y0 + 1, FW = s_hi[1] - x0 + 1;
    if (FH <= 0 || FW <= 0) return;                      // no sample inside the map: no gradient
    if (FH <= RA_PATCH_MAX && FW <= RA_PATCH_MAX && (long)FH * FW <= 4L * q.grid_h * q.grid_w * PP * PP) {
      // per-axis weight sums, in a fixed order (deterministic); 1/count folded into the rows
      roi_align_axis_weights(q.start_h, q.bin_h, q.grid_h, PP, m.H, y0, FH, q.count, s_wy, RA_PATCH_MAX);
      roi_align_axis_weights(q.start_w, q.bin_w, q.grid_w, PP, m.W, x0, FW, 1.f, s_wx, RA_PATCH_MAX);
      __syncthreads();
      for (int c = threadIdx.x; c < g.C; c += 256) {
        float go[PP * PP];
#pragma unroll
        for (int i = 0; i < PP * PP; ++i)
          go[i] = ldf<T>(go_r + (long)c * g.os_c + (long)(i / PP) * g.os_ph + (long)(i % PP) * g.os_pw);
        float* gc = gb + (long)c * m.gs_c + (long)y0 * m.gs_h + (long)x0 * m.gs_w;
        for (int x = 0; x < FW; ++x) {
          float t[PP];                                     // (Go Wx)[:, x]
#pragma unroll
          for (int ph = 0; ph < PP; ++ph) {
            float a = 0.f;
#pragma unroll
            for (int pw = 0; pw < PP; ++pw) a += go[ph * PP + pw] * s_wx[pw * RA_PATCH_MAX + x];
            t[ph] = a;
          }
          for (int y = 0; y < FH; ++y) {
            float v = 0.f;
#pragma unroll
            for (int ph = 0; ph < PP; ++ph) v += s_wy[ph * RA_PATCH_MAX + y] * t[ph];
            if (v != 0.f) atomicAdd(gc + (long)y * m.gs_h + (long)x * m.gs_w, v);
          }
        }
      }
      return;
    }
  }
  // per-sample scatter (large footprints, other pooled sizes)
  for (int c = threadIdx.x; c < g.C; c += 256) {
    float* gc = gb + (long)c * m.gs_c;
    for (int ph = 0; ph < g.PH; ++ph)
      for (int pw = 0; pw < g.PW; ++pw) {
        const float go = ldf<T>(go_r + (long)c * g.os_c + (long)ph * g.os_ph + (long)pw * g.os_pw) / q.count;
        for (int iy = 0; iy < q.grid_h; ++iy) {
          const float y = roi_align_coord(q.start_h, ph, q.bin_h, iy, q.grid_h);
          for (int ix = 0; ix < q.grid_w; ++ix) {
            const float x = roi_align_coord(q.start_w, pw, q.bin_w, ix, q.grid_w);
            Corners k;
            if (!corners(y, x, m.H, m.W, k)) continue;
            atomicAdd(gc + (long)k.yl * m.gs_h + (long)k.xl * m.gs_w, k.w1 * go);
            atomicAdd(gc + (long)k.yl * m.gs_h + (long)k.xh * m.gs_w, k.w2 * go);
            atomicAdd(gc + (long)k.yh * m.gs_h + (long)k.xl * m.gs_w, k.w3 * go);
            atomicAdd(gc + (long)k.yh * m.gs_h + (long)k.xh * m.gs_w, k.w4 * go);
          }
        }
      }
  }
}
#pragma clang fp contract(fast)

}  // namespace relnet

using namespace relnet;

// the forward launch shared by both entries (g.lv / level / num_levels / B filled in)
static int launch_roi_align_fwd(const RoiAlignArgs& g, const void* out, int dtype, void* stream, const char* what) {
  const int groups = g.C / 8;
  bool cl = dtype == RELNET_BF16 && g.C % 8 == 0 && groups <= 256 && 256 % groups == 0 && g.os_c == 1 && g.os_r % 8 == 0 &&
            g.os_ph % 8 == 0 && g.os_pw % 8 == 0 && ((uintptr_t)out & 15) == 0;
  for (int l = 0; l < g.num_levels; ++l)
    cl = cl && g.lv[l].ds_c == 1 && g.lv[l].ds_b % 8 == 0 && g.lv[l].ds_h % 8 == 0 && g.lv[l].ds_w % 8 == 0 && ((uintptr_t)g.lv[l].data & 15) == 0;
  if (cl) {
    const int bins_per_blk = 256 / groups;
    const int bpr = (g.PH * g.PW + bins_per_blk - 1) / bins_per_blk;
    RELNET_REQUIRE((long)g.R * bpr <= INT_MAX, "%s: %d rois exceed the grid", what, g.R);
    roi_align_fwd_cl_kernel<<<dim3((unsigned)(g.R * bpr)), 256, 0, (hipStream_t)stream>>>(g, bpr);
    return check_launch(what);
  }
  RELNET_REQUIRE((long)g.R * g.PH * g.PW <= INT_MAX, "%s: %d rois exceed the grid", what, g.R);
  dim3 grid((unsigned)((long)g.R * g.PH * g.PW));
  if (dtype == RELNET_F32) roi_align_fwd_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else if (dtype == RELNET_BF16) roi_align_fwd_kernel<unsigned short><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else RELNET_REQUIRE(false, "%s: unknown dtype %d", what, dtype);
  return check_launch(what);
}

extern "C" int relnet_roi_align_fwd(const void* data, const long* data_strides4, const float* rois, void* out, const long* out_strides4,
                                    int R, int C, int H, int W, int PH, int PW, float spatial_scale, int sampling_ratio, int aligned,
                                    int batch_index_base, int dtype, void* stream) {
  RELNET_REQUIRE(data && rois && out && data_strides4 && out_strides4, "relnet_roi_align_fwd: null operand");
  RELNET_REQUIRE(R > 0 && C > 0 && H > 0 && W > 0 && PH > 0 && PW > 0, "relnet_roi_align_fwd: bad shape");
  RoiAlignArgs g{};
  g.data = data; g.ds_b = data_strides4[0]; g.ds_c = data_strides4[1]; g.ds_h = data_strides4[2]; g.ds_w = data_strides4[3];
  g.rois = rois; g.out = out; g.os_r = out_strides4[0]; g.os_c = out_strides4[1]; g.os_ph = out_strides4[2]; g.os_pw = out_strides4[3];
  g.R = R; g.C = C; g.H = H; g.W = W; g.PH = PH; g.PW = PW; g.sampling_ratio = sampling_ratio; g.aligned = aligned;
  g.batch_index_base = batch_index_base; g.scale = spatial_scale;
  // one map, no level table; the batch size is not passed here, so only a negative batch index is caught
  g.level = nullptr; g.num_levels = 1; g.B = INT_MAX;
  for (int l = 0; l < 4; ++l) {
    g.lv[l].data = data; g.lv[l].ds_b = g.ds_b; g.lv[l].ds_c = g.ds_c; g.lv[l].ds_h = g.ds_h; g.lv[l].ds_w = g.ds_w;
    g.lv[l].H = H; g.lv[l].W = W; g.lv[l].scale = spatial_scale;
  }
  return launch_roi_align_fwd(g, out, dtype, stream, "relnet_roi_align_fwd");
}

extern "C" int relnet_roi_align_bwd(const void* grad_out, const long* out_strides4, const float* rois, float* grad_in,
                                    const long* grad_in_strides4, int R, int C, int H, int W, int PH, int PW, float spatial_scale,
                                    int sampling_ratio, int aligned, int batch_index_base, int dtype, void* stream) {
  RELNET_REQUIRE(grad_out && rois && grad_in && out_strides4 && grad_in_strides4, "relnet_roi_align_bwd: null operand");
  RELNET_REQUIRE(R > 0 && C > 0 && H > 0 && W > 0 && PH > 0 && PW > 0, "relnet_roi_align_bwd: bad shape");
  RoiAlignArgs g{};
  g.rois = rois; g.out = const_cast<void*>(grad_out); g.os_r = out_strides4[0]; g.os_c = out_strides4[1]; g.os_ph = out_strides4[2]; g.os_pw = out_strides4[3];
  g.grad_in = grad_in; g.gs_b = grad_in_strides4[0]; g.gs_c = grad_in_strides4[1]; g.gs_h = grad_in_strides4[2]; g.gs_w = grad_in_strides4[3];
  g.R = R; g.C = C; g.H = H; g.W = W; g.PH = PH; g.PW = PW; g.sampling_ratio = sampling_ratio; g.aligned = aligned;
  g.batch_index_base = batch_index_base; g.scale = spatial_scale;
  dim3 grid((unsigned)((long)R * PH * PW));
  if (dtype == RELNET_F32) roi_align_bwd_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else if (dtype == RELNET_BF16) roi_align_bwd_kernel<unsigned short><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else RELNET_REQUIRE(false, "relnet_roi_align_bwd: unknown dtype %d", dtype);
  return check_launch("relnet_roi_align_bwd");
}

// levels entries: host arrays of num_levels (1..4) maps; levels past num_levels repeat the last one (never selected: level out of range
// means zeros).  Per-level strides in elements, (b, c, y, x).
static int fill_levels(RoiAlignArgs& g, const long* strides4_levels, const int* heights, const int* widths, const float* spatial_scales,
                       int num_levels, const char* what) {
  RELNET_REQUIRE(strides4_levels && heights && widths && spatial_scales, "%s: null operand", what);
  RELNET_REQUIRE(num_levels >= 1 && num_levels <= 4, "%s: 1..4 pyramid levels, got %d", what, num_levels);
  if (roi_fill_levels(num_levels, [&](int l, int s) {
    RELNET_REQUIRE(heights[s] > 0 && widths[s] > 0, "%s: bad level %d", what, s);
    g.lv[l].H = heights[s]; g.lv[l].W = widths[s]; g.lv[l].scale = spatial_scales[s];
    return 0;
  })) return -1;
  g.num_levels = num_levels;
  return 0;
}

extern "C" int relnet_roi_align_levels_fwd(const void* const* data_levels, const long* data_strides4_levels, const int* heights,
                                           const int* widths, const float* spatial_scales, int num_levels, const float* rois,
                                           const int* roi_level, void* out, const long* out_strides4, int R, int B, int C, int PH, int PW,
                                           int sampling_ratio, int aligned, int batch_index_base, int dtype, void* stream) {
  const char* what = "relnet_roi_align_levels_fwd";
  RELNET_REQUIRE(data_levels && rois && out && out_strides4, "%s: null operand", what);
  RELNET_REQUIRE(R >= 0 && B > 0 && C > 0 && PH > 0 && PW > 0, "%s: bad shape", what);
  RoiAlignArgs g{};
  if (fill_levels(g, data_strides4_levels, heights, widths, spatial_scales, num_levels, what)) return -1;
  if (roi_fill_levels(num_levels, [&](int l, int s) {
    RELNET_REQUIRE(data_levels[s], "%s: null level %d", what, s);
    g.lv[l].data = data_levels[s]; g.lv[l].ds_b = data_strides4_levels[4 * s]; g.lv[l].ds_c = data_strides4_levels[4 * s + 1];
    g.lv[l].ds_h = data_strides4_levels[4 * s + 2]; g.lv[l].ds_w = data_strides4_levels[4 * s + 3];
    return 0;
  })) return -1;
  g.rois = rois; g.out = out; g.os_r = out_strides4[0]; g.os_c = out_strides4[1]; g.os_ph = out_strides4[2]; g.os_pw = out_strides4[3];
  g.R = R; g.C = C; g.PH = PH; g.PW = PW; g.sampling_ratio = sampling_ratio; g.aligned = aligned;
  g.batch_index_base = batch_index_base; g.level = roi_level; g.B = B;
  if (R == 0) return 0;
  return launch_roi_align_fwd(g, out, dtype, stream, what);
}

extern "C" int relnet_roi_align_levels_bwd(const void* grad_out, const long* out_strides4, const float* rois, const int* roi_level,
                                           float* const* grad_levels, const long* grad_strides4_levels, const int* heights, const int* widths,
                                           const float* spatial_scales, int num_levels, int R, int B, int C, int PH, int PW,
                                           int sampling_ratio, int aligned, int batch_index_base, int dtype, void* stream) {
  const char* what = "relnet_roi_align_levels_bwd";
  RELNET_REQUIRE(grad_out && out_strides4 && rois && grad_levels, "%s: null operand", what);
  RELNET_REQUIRE(R >= 0 && B > 0 && C > 0 && PH > 0 && PW > 0, "%s: bad shape", what);
  RoiAlignArgs g{};
  if (fill_levels(g, grad_strides4_levels, heights, widths, spatial_scales, num_levels, what)) return -1;
  if (roi_fill_levels(num_levels, [&](int l, int s) {
    RELNET_REQUIRE(grad_levels[s], "%s: null level %d", what, s);
    g.lv[l].grad = grad_levels[s]; g.lv[l].gs_b = grad_strides4_levels[4 * s]; g.lv[l].gs_c = grad_strides4_levels[4 * s + 1];
    g.lv[l].gs_h = grad_strides4_levels[4 * s + 2]; g.lv[l].gs_w = grad_strides4_levels[4 * s + 3];
    return 0;
  })) return -1;
  g.rois = rois; g.out = const_cast<void*>(grad_out);
  g.os_r = out_strides4[0]; g.os_c = out_strides4[1]; g.os_ph = out_strides4[2]; g.os_pw = out_strides4[3];
  g.R = R; g.C = C; g.PH = PH; g.PW = PW; g.sampling_ratio = sampling_ratio; g.aligned = aligned;
  g.batch_index_base = batch_index_base; g.level = roi_level; g.B = B;
  if (R == 0) return 0;
  const dim3 grid((unsigned)R);
  const bool p7 = PH == 7 && PW == 7;
  if (dtype == RELNET_F32) {
    if (p7) roi_align_bwd_levels_kernel<float, 7><<<grid, 256, 0, (hipStream_t)stream>>>(g);
    else roi_align_bwd_levels_kernel<float, 0><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  } else if (dtype == RELNET_BF16) {
    if (p7) roi_align_bwd_levels_kernel<unsigned short, 7><<<grid, 256, 0, (hipStream_t)stream>>>(g);
    else roi_align_bwd_levels_kernel<unsigned short, 0><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  } else RELNET_REQUIRE(false, "%s: unknown dtype %d", what, dtype);
  return check_launch(what);
}
