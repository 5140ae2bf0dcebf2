// Image pre-processing on the device, from decoded uint8 BGR HWC sources (lib/utils/image.py:16-129 of the reference, restated in
// numpy by dataset/image.py): the bilinear resize (cv2 INTER_LINEAR, image.py:88-116) into a zero-filled per-batch canvas, and the
// unfused transform (mean subtraction + BGR -> RGB NCHW, image.py:118-129, with tensor_vstack's zero batch padding).
// The resize is bit-identical to dataset/image.py:resize: the same float64 operations in the same order, no contraction.
#include "common.h"

namespace relnet {

struct ResizeU8Args {
  const unsigned char* src;     // B sources back to back, each [h, w, 3] BGR HWC
  long src_bytes;
  const long* table;            // [B, 6]: byte offset, h, w, flip, nh, nw
  const double* scale;          // [B]: im_scale
  unsigned char* out;           // [B, Hc, Wc, 3]
  int B, Hc, Wc;
};

#pragma clang fp contract(off)
// dataset/image.py:_bilinear_axis for one destination position: (left index, right index, weight of the right tap)
__device__ __forceinline__ void bilinear_tap(int d, int n_src, double scale, int& i0, int& i1, double& w1) {
  const double f = ((double)d + 0.5) / scale - 0.5;
  double fl = floor(f);
  w1 = f - fl;
  if (fl < 0.0) { fl = 0.0; w1 = 0.0; }
  if (fl >= (double)(n_src - 1)) { fl = (double)(n_src - 1); w1 = 0.0; }
  i0 = (int)fl;
  i1 = min(i0 + 1, n_src - 1);
}

__global__ __launch_bounds__(256) void resize_u8_kernel(ResizeU8Args g) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)g.B * g.Hc * g.Wc;
  if (t >= total) return;
  const int x = (int)(t % g.Wc);
  long p = t / g.Wc;
  const int y = (int)(p % g.Hc);
  const int b = (int)(p / g.Hc);
  const long* row = g.table + 6 * (long)b;
  const long off = row[0];
  const int h = (int)row[1], w = (int)row[2], flip = (int)row[3], nh = (int)row[4], nw = (int)row[5];
  unsigned char* o = g.out + t * 3;
  // pixels outside the resized image (and every pixel of an entry that does not describe a source inside the buffer) are 0
  if (y >= nh || x >= nw || h <= 0 || w <= 0 || off < 0 || off + (long)h * w * 3 > g.src_bytes) {
    o[0] = 0; o[1] = 0; o[2] = 0;
    return;
  }
  const double s = g.scale[b];
  int x0, x1, y0, y1;
  double wx, wy;
  bilinear_tap(x, w, s, x0, x1, wx);
  bilinear_tap(y, h, s, y0, y1, wy);
  if (flip) { x0 = w - 1 - x0; x1 = w - 1 - x1; }      // get_image's im[:, ::-1, :] before the resize
  const unsigned char* im = g.src + off;
  const unsigned char* a0 = im + ((long)y0 * w + x0) * 3;
  const unsigned char* a1 = im + ((long)y0 * w + x1) * 3;
  const unsigned char* b0 = im + ((long)y1 * w + x0) * 3;
  const unsigned char* b1 = im + ((long)y1 * w + x1) * 3;
  const double vx = 1.0 - wx, vy = 1.0 - wy;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double top = (double)a0[c] * vx + (double)a1[c] * wx;
    const double bot = (double)b0[c] * vx + (double)b1[c] * wx;
    const double v = rint(top * vy + bot * wy);                       // np.rint: half to even
    o[c] = (unsigned char)fmin(fmax(v, 0.0), 255.0);
  }
}

struct TransformU8Args {
  const unsigned char* data;    // [B, H, W, 3] BGR HWC
  const float* im_info;         // [B, 3] or null
  void* out;                    // [B, 3, H, W] RGB NCHW fp32 / bf16
  int out_bf16, B, H, W;
  double mean[3];               // BGR
};

// one thread per (b, y, x): three loads of one pixel, three plane stores
__global__ __launch_bounds__(256) void image_transform_u8_kernel(TransformU8Args g) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long plane = (long)g.H * g.W;
  if (t >= (long)g.B * plane) return;
  const int x = (int)(t % g.W);
  const long p = t / g.W;
  const int y = (int)(p % g.H);
  const int b = (int)(p / g.H);
  int eh = g.H, ew = g.W;
  if (g.im_info) { eh = min(eh, (int)g.im_info[3 * b]); ew = min(ew, (int)g.im_info[3 * b + 1]); }
  const bool in = y < eh && x < ew;
  const unsigned char* px = g.data + t * 3;
  const long o = (long)b * 3 * plane + (long)y * g.W + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {                                           // RGB channel c <- BGR byte 2 - c
    const float v = in ? (float)((double)px[2 - c] - g.mean[2 - c]) : 0.f;   // exact in double, one rounding to float
    if (g.out_bf16) ((unsigned short*)g.out)[o + c * plane] = f2bf(v);
    else ((float*)g.out)[o + c * plane] = v;
  }
}
#pragma clang fp contract(on)

}  // namespace relnet

using namespace relnet;

extern "C" int relnet_resize_u8(const void* src, long src_bytes, const long* table, const double* scale, void* out, int B, int Hc,
                                int Wc, void* stream) {
  RELNET_REQUIRE(src && table && scale && out, "relnet_resize_u8: null operand");
  RELNET_REQUIRE(B > 0 && Hc > 0 && Wc > 0 && src_bytes > 0, "relnet_resize_u8: bad shape");
  ResizeU8Args g{(const unsigned char*)src, src_bytes, table, scale, (unsigned char*)out, B, Hc, Wc};
  const long total = (long)B * Hc * Wc;
  resize_u8_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(g);
  return check_launch("relnet_resize_u8");
}

extern "C" int relnet_image_transform_u8(const void* data, const float* im_info, double mean_b, double mean_g, double mean_r,
                                         void* out, int out_dtype, int B, int H, int W, void* stream) {
  RELNET_REQUIRE(data && out, "relnet_image_transform_u8: null operand");
  RELNET_REQUIRE(B > 0 && H > 0 && W > 0 && (out_dtype == 0 || out_dtype == 1), "relnet_image_transform_u8: bad shape");
  TransformU8Args g;
  g.data = (const unsigned char*)data; g.im_info = im_info; g.out = out; g.out_bf16 = out_dtype == 1;
  g.B = B; g.H = H; g.W = W;
  g.mean[0] = mean_b; g.mean[1] = mean_g; g.mean[2] = mean_r;
  const long total = (long)B * H * W;
  image_transform_u8_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(g);
  return check_launch("relnet_image_transform_u8");
}
