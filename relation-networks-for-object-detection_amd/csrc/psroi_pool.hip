// PSROIPooling forward / backward: `_contrib_PSROIPooling` of relation_rcnn/operator_cxx (psroi_pooling.cu:32-101 forward, :132-194
// backward; parameters psroi_pooling-inl.h:36-46), the position-sensitive average pooling of R-FCN.
//
//   per output element (n, ctop, ph, pw), P = pooled_size, g = group_size, all in fp32, every product and sum rounded on its own:
//   start_w = roundf(x1) * scale, end_w = (roundf(x2) + 1) * scale          (roundf: halves away from zero; likewise h from y1 / y2)
//   roi_w = max(end_w - start_w, 0.1), bin_w = roi_w / P
//   wstart = clip(floor(pw * bin_w + start_w), 0, W), wend = clip(ceil((pw + 1) * bin_w + start_w), 0, W)      (clipped as floats, so a
//                                                                             wild coordinate is a defined, in-range window)
//   gw = clamp(floor(float(pw) * g / P), 0, g - 1), gh likewise, c = (ctop * g + gh) * g + gw
//   out = hend <= hstart || wend <= wstart ? 0 : (sum of data[b][c][h][w] over the window) / ((hend - hstart) * (wend - wstart))
//
// SUMMATION ORDER (part of the contract, include/relnet_hip.h):
//   forward:  one thread owns one output element and adds its window's cells to 0 with h ascending, then w ascending (the reference's
//             order), in fp32; one IEEE division by the cell count; a bf16 output is rounded once, after it.
//   backward: one thread owns one word of grad_in (image, channel, cell) and adds to 0, in ascending (roi, ph, pw) order, the value
//             grad_out[n][ctop][ph][pw] / bin_area (one IEEE fp32 division each) of every bin that holds the cell and maps to the channel.
//             No atomics, global or LDS.  The word is then written (accumulate == 0) or added to its old value with one addition.
//   Neither order depends on the grid, the CU count, the layout or the alignment of an operand.
//
// A roi whose batch index (minus batch_index_base) lies outside [0, B) pools to zeros and contributes no gradient; the test comes before
// any address is formed (the reference reads out of bounds).  All extents are folded into grid.x.
#include "common.h"

namespace relnet {

struct PsroiArgs {
  const void* data; long ds_b, ds_c, ds_h, ds_w;       // forward: [B, C, H, W] element strides
  const float* rois;                                    // [R, 5] batch_idx, x1, y1, x2, y2
  void* out; long os_r, os_c, os_ph, os_pw;             // forward: output; backward: the output GRADIENT; logical [R, OD, P, P]
  float* mapping;                                       // forward: optional second output (the channel c), out's strides
  float* grad_in; long gs_b, gs_c, gs_h, gs_w;          // backward: fp32 [B, C, H, W]
  int R, B, C, H, W, OD, P, G, batch_index_base, accumulate;
  int c_fast;                                           // forward thread order: channel fastest (channels-last output) or pw fastest
  float scale;
  long total;                                           // forward: output elements
};

#pragma clang fp contract(off)
struct PsroiGeom { long b; float start_h, start_w, bin_h, bin_w; };

__device__ __forceinline__ PsroiGeom psroi_geom(const float* roi, float scale, int P, int batch_index_base) {
  PsroiGeom q;
  q.b = (long)(int)roi[0] - batch_index_base;
  q.start_w = roundf(roi[1]) * scale; q.start_h = roundf(roi[2]) * scale;
  const float end_w = (roundf(roi[3]) + 1.f) * scale, end_h = (roundf(roi[4]) + 1.f) * scale;
  const float rw = fmaxf(end_w - q.start_w, 0.1f), rh = fmaxf(end_h - q.start_h, 0.1f);      // avoid 0
  q.bin_h = rh / (float)P; q.bin_w = rw / (float)P;
  return q;
}
// cells [s, e) of bin p along one axis of a map of extent L (e <= s: the bin is empty)
__device__ __forceinline__ void psroi_span(int p, float bin, float start, int L, int& s, int& e) {
  s = (int)fminf(fmaxf(floorf((float)p * bin + start), 0.f), (float)L);
  e = (int)fminf(fmaxf(ceilf((float)(p + 1) * bin + start), 0.f), (float)L);
}
// group row / column of bin p
__device__ __forceinline__ int psroi_group(int p, int G, int P) {
  return min(max((int)floorf((float)p * (float)G / (float)P), 0), G - 1);
}

// thread = one output element; any strides, T = float | bf16 bits
template <typename T>
__global__ __launch_bounds__(256) void psroi_pool_fwd_kernel(PsroiArgs g) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.total) return;
  int pw, ph, ctop, r;
  if (g.c_fast) {
    ctop = (int)(i % g.OD); pw = (int)((i / g.OD) % g.P); ph = (int)((i / g.OD / g.P) % g.P); r = (int)(i / g.OD / g.P / g.P);
  } else {
    pw = (int)(i % g.P); ph = (int)((i / g.P) % g.P); ctop = (int)((i / g.P / g.P) % g.OD); r = (int)(i / g.P / g.P / g.OD);
  }
  const PsroiGeom q = psroi_geom(g.rois + (long)r * 5, g.scale, g.P, g.batch_index_base);
  const int c = (ctop * g.G + psroi_group(ph, g.G, g.P)) * g.G + psroi_group(pw, g.G, g.P);
  float v = 0.f;
  if (q.b >= 0 && q.b < g.B) {
    int hs, he, ws, we;
    psroi_span(ph, q.bin_h, q.start_h, g.H, hs, he);
    psroi_span(pw, q.bin_w, q.start_w, g.W, ws, we);
    if (he > hs && we > ws) {
      const T* p = (const T*)g.data + q.b * g.ds_b + (long)c * g.ds_c;
      float sum = 0.f;
      for (int h = hs; h < he; ++h)
        for (int w = ws; w < we; ++w) sum += ldf<T>(p + (long)h * g.ds_h + (long)w * g.ds_w);
      v = sum / (float)((he - hs) * (we - ws));
    }
  }
  const long o = (long)r * g.os_r + (long)ctop * g.os_c + (long)ph * g.os_ph + (long)pw * g.os_pw;
  stf<T>((T*)g.out + o, v);
  if (g.mapping) g.mapping[o] = (float)c;
}

// Backward, gather form: thread = one word of grad_in, workgroup = one cell (image, y, x) x 256 consecutive channels.  Which of a roi's
// bins hold the cell does not depend on the channel, so the workgroup finds that once per roi, 256 rois at a time: thread t evaluates roi
// r0 + t (psroi_geom / psroi_span, the forward's own functions, so both directions see the same bits) and finds the bin ranges
// [pha, phb] x [pwa, pwb] that hold the cell (the bins that hold a coordinate are consecutive: both edges of psroi_span are monotone
// in p); a roi of another image, with a bad batch index or off the cell is a miss.  The hits are compacted into LDS in ascending roi order
// (ballot + prefix count: no atomics), and every thread walks that list.  Of the bins that hold the cell only those in the group row /
// column of the thread's channel feed it: [ph0, ph1] x [pw0, pw1], found once per thread (psroi_group is monotone in p too).  Adjacent
// bins overlap (floor / ceil) and P > g gives several bins per channel, so the whole intersection is summed, ph ascending, then pw.
template <typename T>
__global__ __launch_bounds__(256) void psroi_pool_bwd_kernel(PsroiArgs g, int chunks) {
  __shared__ float s_geom[256][4];
  __shared__ int s_rng[256][4];
  __shared__ int s_roi[256];
  __shared__ int s_cnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = (int)(blockIdx.x % chunks) * 256 + threadIdx.x;
  const long cell = blockIdx.x / chunks;
  const int x = (int)(cell % g.W), y = (int)((cell / g.W) % g.H), b = (int)(cell / g.W / g.H);
  const bool live = c < g.C;
  const int gw = c % g.G, gh = (c / g.G) % g.G, ctop = c / (g.G * g.G);
  int ph0 = g.P, ph1 = -1, pw0 = g.P, pw1 = -1;
  for (int p = 0; p < g.P; ++p) {
    const int q = psroi_group(p, g.G, g.P);
    if (q == gh) { ph0 = min(ph0, p); ph1 = p; }
    if (q == gw) { pw0 = min(pw0, p); pw1 = p; }
  }
  float acc = 0.f;
  for (int r0 = 0; r0 < g.R; r0 += 256) {
    const int r = r0 + threadIdx.x;
    PsroiGeom q{};
    int pha = -1, phb = -1, pwa = -1, pwb = -1;
    if (r < g.R) {
      q = psroi_geom(g.rois + (long)r * 5, g.scale, g.P, g.batch_index_base);
      if (q.b == b) {                                     // b is in [0, B): a bad batch index matches no workgroup
        for (int p = 0; p < g.P; ++p) {
          int s, e;
          psroi_span(p, q.bin_h, q.start_h, g.H, s, e);
          if (y >= s && y < e) { if (pha < 0) pha = p; phb = p; }
          psroi_span(p, q.bin_w, q.start_w, g.W, s, e);
          if (x >= s && x < e) { if (pwa < 0) pwa = p; pwb = p; }
        }
      }
    }
    const bool hit = pha >= 0 && pwa >= 0;
    const unsigned long long m = __ballot(hit);
    __syncthreads();                                      // the previous list has been read
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int at = 0, n = 0;
    for (int w = 0; w < 4; ++w) { at += w < wave ? s_cnt[w] : 0; n += s_cnt[w]; }
    if (hit) {
      at += __popcll(m & ((1ull << lane) - 1ull));
      s_geom[at][0] = q.start_h; s_geom[at][1] = q.start_w; s_geom[at][2] = q.bin_h; s_geom[at][3] = q.bin_w;
      s_rng[at][0] = pha; s_rng[at][1] = phb; s_rng[at][2] = pwa; s_rng[at][3] = pwb;
      s_roi[at] = r;
    }
    __syncthreads();
    if (!live) continue;
    for (int k = 0; k < n; ++k) {
      const int pa = max(ph0, s_rng[k][0]), pb = min(ph1, s_rng[k][1]), qa = max(pw0, s_rng[k][2]), qb = min(pw1, s_rng[k][3]);
      if (pa > pb || qa > qb) continue;
      const float start_h = s_geom[k][0], start_w = s_geom[k][1], bin_h = s_geom[k][2], bin_w = s_geom[k][3];
      const T* go = (const T*)g.out + (long)s_roi[k] * g.os_r + (long)ctop * g.os_c;
      for (int ph = pa; ph <= pb; ++ph) {
        int hs, he;
        psroi_span(ph, bin_h, start_h, g.H, hs, he);
        for (int pw = qa; pw <= qb; ++pw) {
          int ws, we;
          psroi_span(pw, bin_w, start_w, g.W, ws, we);
          acc += ldf<T>(go + (long)ph * g.os_ph + (long)pw * g.os_pw) / (float)((he - hs) * (we - ws));
        }
      }
    }
  }
  if (!live) return;
  float* dst = g.grad_in + (long)b * g.gs_b + (long)c * g.gs_c + (long)y * g.gs_h + (long)x * g.gs_w;
  *dst = g.accumulate ? *dst + acc : acc;
}
#pragma clang fp contract(fast)

}  // namespace relnet

using namespace relnet;

static int psroi_check(const char* what, int R, int B, int C, int H, int W, int output_dim, int pooled_size, int group_size, int dtype) {
  RELNET_REQUIRE(pooled_size > 0 && group_size > 0 && output_dim > 0, "%s: pooled_size %d, group_size %d and output_dim %d must be positive",
                 what, pooled_size, group_size, output_dim);
  RELNET_REQUIRE(R >= 0 && B > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape", what);
  RELNET_REQUIRE((long)output_dim * group_size * group_size == (long)C, "%s: %d channels != output_dim %d * group_size %d^2", what, C,
                 output_dim, group_size);
  RELNET_REQUIRE(dtype == RELNET_F32 || dtype == RELNET_BF16, "%s: unknown dtype %d", what, dtype);
  return 0;
}

extern "C" int relnet_psroi_pool_fwd(const void* data, const long* data_strides4, const float* rois, void* out, const long* out_strides4,
                                     float* mapping_channel, int R, int B, int C, int H, int W, int output_dim, int pooled_size,
                                     int group_size, float spatial_scale, int batch_index_base, int dtype, void* stream) {
  const char* what = "relnet_psroi_pool_fwd";
  if (psroi_check(what, R, B, C, H, W, output_dim, pooled_size, group_size, dtype)) return -1;
  RELNET_REQUIRE(data_strides4 && out_strides4 && (R == 0 || (data && rois && out)), "%s: null operand", what);
  if (R == 0) return 0;
  PsroiArgs g{};
  g.data = data; g.ds_b = data_strides4[0]; g.ds_c = data_strides4[1]; g.ds_h = data_strides4[2]; g.ds_w = data_strides4[3];
  g.rois = rois; g.out = out; g.os_r = out_strides4[0]; g.os_c = out_strides4[1]; g.os_ph = out_strides4[2]; g.os_pw = out_strides4[3];
  g.mapping = mapping_channel;
  g.R = R; g.B = B; g.C = C; g.H = H; g.W = W; g.OD = output_dim; g.P = pooled_size; g.G = group_size;
  g.batch_index_base = batch_index_base; g.scale = spatial_scale; g.c_fast = g.os_c == 1 && output_dim > 1;
  g.total = (long)R * output_dim * pooled_size * pooled_size;
  const long blocks = (g.total + 255) / 256;
  RELNET_REQUIRE(blocks <= INT_MAX, "%s: %ld output elements exceed the grid", what, g.total);
  if (dtype == RELNET_F32) psroi_pool_fwd_kernel<float><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(g);
  else psroi_pool_fwd_kernel<unsigned short><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(g);
  return check_launch(what);
}

extern "C" int relnet_psroi_pool_bwd(const void* grad_out, const long* out_strides4, const float* rois, float* grad_in,
                                     const long* grad_in_strides4, int R, int B, int C, int H, int W, int output_dim, int pooled_size,
                                     int group_size, float spatial_scale, int batch_index_base, int accumulate, int dtype, void* stream) {
  const char* what = "relnet_psroi_pool_bwd";
  if (psroi_check(what, R, B, C, H, W, output_dim, pooled_size, group_size, dtype)) return -1;
  RELNET_REQUIRE(out_strides4 && grad_in_strides4 && grad_in && (R == 0 || (grad_out && rois)), "%s: null operand", what);
  if (R == 0 && accumulate) return 0;                   // nothing to add; without accumulate the kernel still writes the zeros
  PsroiArgs g{};
  g.rois = rois; g.out = const_cast<void*>(grad_out);
  g.os_r = out_strides4[0]; g.os_c = out_strides4[1]; g.os_ph = out_strides4[2]; g.os_pw = out_strides4[3];
  g.grad_in = grad_in; g.gs_b = grad_in_strides4[0]; g.gs_c = grad_in_strides4[1]; g.gs_h = grad_in_strides4[2]; g.gs_w = grad_in_strides4[3];
  g.R = R; g.B = B; g.C = C; g.H = H; g.W = W; g.OD = output_dim; g.P = pooled_size; g.G = group_size;
  g.batch_index_base = batch_index_base; g.accumulate = accumulate; g.scale = spatial_scale;
  const int chunks = (C + 255) / 256;
  const long blocks = (long)B * H * W * chunks;
  RELNET_REQUIRE(blocks <= INT_MAX, "%s: %ld workgroups exceed the grid", what, blocks);
  if (dtype == RELNET_F32) psroi_pool_bwd_kernel<float><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(g, chunks);
  else psroi_pool_bwd_kernel<unsigned short><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(g, chunks);
  return check_launch(what);
}
