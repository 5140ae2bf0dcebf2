// Backward of the stem (reference graph: conv1 -> bn_conv1 -> conv1_relu -> pool1, relation_rcnn/symbols/resnet_v1_101_rcnn_base.py:30-36),
// for a training step whose network.FIXED_PARAMS leaves conv1 trainable: the adjoint of relnet_stem_bias_relu_pool and the weight gradient
// of the 7x7 / 2 convolution.  conv1 reads the image, so there is no data gradient.  Neither kernel uses a float atomic: both give the same
// bits on every run, and cfg.deterministic needs no second form of them.
#include "common.h"

namespace relnet {

// ---------------------------------------------------------------------------------------
// relnet_stem_pool_bwd: out = relu(maxpool_ceil(conv) + bias), 3x3 window, stride 2, pooling_convention='full' (windows clipped at the
// bottom / right border exactly as stem_bias_relu_pool_kernel clips them).  A window hands d_out * (out > 0) to its FIRST maximum in
// row-major window order -- MXNet's unpool rule (mshadow unpool<red::maximum> visits the window in that order and stops at the first
// equal element) and torch's max_pool2d backward.  Like ROIPooling's, this is a restatement: the reference repository has no pooling
// source of its own to run.
// Written as a gather: one thread owns one conv pixel x one group of channels, visits the at most 2 x 2 windows that cover the pixel in
// ascending (ph, pw), sums in fp32 from 0 and rounds once.  No zero fill, no atomics, every word of d_conv is written exactly once.
// ---------------------------------------------------------------------------------------
template <typename T> struct PoolBwdVec;
template <> struct PoolBwdVec<unsigned short> {
  static constexpr int V = 8;
  static __device__ __forceinline__ void load(const unsigned short* p, float* v) {
    const uint4 q = *(const uint4*)p;
    const unsigned int w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = bf2f(w4[e] & 0xffff); v[2 * e + 1] = bf2f(w4[e] >> 16); }
  }
  static __device__ __forceinline__ void store(unsigned short* p, const float* v) {
    *(uint4*)p = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
  }
};
template <> struct PoolBwdVec<float> {
  static constexpr int V = 4;
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const float4 q = *(const float4*)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  }
  static __device__ __forceinline__ void store(float* p, const float* v) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
};

template <typename T> struct StemPoolBwdArgs {
  const T* conv;     // [B, H, W, C] conv map before bias
  const T* out;      // [B, Ho, Wo, C] pooled output (after bias + ReLU)
  const T* d_out;    // [B, Ho, Wo, C]
  T* d_conv;         // [B, H, W, C]
  int B, H, W, C, Ho, Wo;
};

template <typename T> __global__ __launch_bounds__(256) void stem_pool_bwd_kernel(StemPoolBwdArgs<T> g) {
  constexpr int V = PoolBwdVec<T>::V;
  const int groups = g.C / V;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)g.B * g.H * g.W * groups) return;
  const int cg = (int)(t % groups);
  long p = t / groups;
  const int x = (int)(p % g.W); p /= g.W;
  const int y = (int)(p % g.H);
  const int b = (int)(p / g.H);
  const T* base = g.conv + (long)b * g.H * g.W * g.C + cg * V;
  float mine[V], sum[V];
  PoolBwdVec<T>::load(base + ((long)y * g.W + x) * g.C, mine);
#pragma unroll
  for (int e = 0; e < V; ++e) sum[e] = 0.f;
  // windows ph with 2 ph <= y <= 2 ph + 2 (those that exist), likewise pw
  const int ph_lo = y > 0 ? (y - 1) >> 1 : 0, ph_hi = min(y >> 1, g.Ho - 1);
  const int pw_lo = x > 0 ? (x - 1) >> 1 : 0, pw_hi = min(x >> 1, g.Wo - 1);
  for (int ph = ph_lo; ph <= ph_hi; ++ph)
    for (int pw = pw_lo; pw <= pw_hi; ++pw) {
      const int y0 = 2 * ph, x0 = 2 * pw;
      const int y1 = min(y0 + 3, g.H), x1 = min(x0 + 3, g.W);        // the forward's own clipping
      bool first[V];
#pragma unroll
      for (int e = 0; e < V; ++e) first[e] = true;
      for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
          if (yy == y && xx == x) continue;
          float v[V];
          PoolBwdVec<T>::load(base + ((long)yy * g.W + xx) * g.C, v);
          const bool before = yy < y || (yy == y && xx < x);          // row-major window order
#pragma unroll
          for (int e = 0; e < V; ++e) first[e] = first[e] && (before ? v[e] < mine[e] : v[e] <= mine[e]);
        }
      const long o = (((long)b * g.Ho + ph) * g.Wo + pw) * g.C + cg * V;
      float ov[V], dv[V];
      PoolBwdVec<T>::load(g.out + o, ov);
      PoolBwdVec<T>::load(g.d_out + o, dv);
#pragma unroll
      for (int e = 0; e < V; ++e) sum[e] += (first[e] && ov[e] > 0.f) ? dv[e] : 0.f;
    }
  PoolBwdVec<T>::store(g.d_conv + (((long)b * g.H + y) * g.W + x) * g.C + cg * V, sum);
}

// ---------------------------------------------------------------------------------------
// relnet_stem_wgrad: dW[64][7 * 7 * 3] += scale^2 * sum over pixels of d_conv[p, :]^T patch[p, :] for the 7x7 / 2 / pad 3 convolution,
// read from the packed image of relnet_stem_pack_input (zero-padded NHWC4 bf16: the 8 taps x 4 channels of one window row are 32
// contiguous elements; tap 7, tap row 7 and channel 3 are computed and dropped).  The product is [64 channels] x [256 = ty*32 + tx*4 + c]
// (the layout of ops.pack_stem_weight) with the PIXELS as the reduction index, on v_mfma_f32_32x32x16_bf16: both operands have the
// reduction index as their slow axis in memory, so each stage of 64 pixels is transposed through LDS ([channel][pixel], [k][pixel]) and
// read back as 16-byte fragments.
// The pixels are cut into chunks of kSwChunk: the chunk count depends on (B, Hc, Wc) only, never on the device.  A workgroup sums its
// chunk in pixel order into registers and writes one [64][256] fp32 partial; a second kernel adds the partials in ascending chunk order
// into dW.  No atomics, one order: the result is the same bits on every run.
// ---------------------------------------------------------------------------------------
constexpr int kSwChunk = 4096;              // pixels per partial sum
constexpr int kSwSub = 64;                  // pixels per LDS stage (4 k-steps of 16)
constexpr int kSwLd = kSwSub + 8;           // LDS row pitch in elements: 144 B (16-byte aligned fragments)

struct StemWgradArgs {
  const unsigned short* packed;   // [B, Hp, Wp, 4] bf16
  const unsigned short* d_conv;   // [B * Hc * Wc, 64] bf16
  float* part;                    // [chunks][64][256]
  long P;                         // B * Hc * Wc
  int Hp, Wp, Hc, Wc;
};

__global__ __launch_bounds__(256) void stem_wgrad_partial_kernel(StemWgradArgs g) {
  __shared__ __attribute__((aligned(16))) unsigned short sD[64 * kSwLd];      // [channel][pixel]
  __shared__ __attribute__((aligned(16))) unsigned short sP[256 * kSwLd];     // [k = ty*32 + tx*4 + c][pixel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const long p_begin = (long)blockIdx.x * kSwChunk;
  const long p_end = min(p_begin + (long)kSwChunk, g.P);
  f32x16 acc[2][2];                                              // [channel tile][k tile 2 wave + j]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  for (long p0 = p_begin; p0 < p_end; p0 += kSwSub) {
    // ---- d_conv rows -> sD[channel][pixel]; pixels past the chunk's end contribute zeros
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + 256 * it;
      const int cg = idx >> 6, pl = idx & 63;                    // consecutive lanes: consecutive pixels (LDS stores of one row)
      const long p = p0 + pl;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (p < p_end) v = *(const uint4*)(g.d_conv + p * 64 + cg * 8);
      const unsigned int w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sD[(cg * 8 + 2 * e) * kSwLd + pl] = (unsigned short)(w4[e] & 0xffff);
        sD[(cg * 8 + 2 * e + 1) * kSwLd + pl] = (unsigned short)(w4[e] >> 16);
      }
    }
    // ---- window rows -> sP[k][pixel]: tap row ty of pixel (b, cy, cx) is 32 contiguous elements at packed[b][2 cy + ty][2 cx]
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + 256 * it;
      const int ty = idx >> 6, pl = idx & 63;
      const long p = p0 + pl;
      uint4 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = make_uint4(0u, 0u, 0u, 0u);
      if (p < p_end) {
        const int cx = (int)(p % g.Wc);
        const long q_ = p / g.Wc;
        const int cy = (int)(q_ % g.Hc);
        const long b = q_ / g.Hc;
        const unsigned short* src = g.packed + ((b * g.Hp + 2 * cy + ty) * g.Wp + 2 * cx) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *(const uint4*)(src + 8 * q);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned int w4[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sP[(ty * 32 + q * 8 + 2 * e) * kSwLd + pl] = (unsigned short)(w4[e] & 0xffff);
          sP[(ty * 32 + q * 8 + 2 * e + 1) * kSwLd + pl] = (unsigned short)(w4[e] >> 16);
        }
      }
    }
    __syncthreads();
    // ---- D[channel][k] += A[channel][pixel] B[pixel][k]: lane (r = l & 31, h = l >> 5) holds A[r][8 h + j], B[8 h + j][r]
#pragma unroll
    for (int ks = 0; ks < kSwSub / 16; ++ks) {
      bf16x8 af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = *(const bf16x8*)(sD + (32 * i + l31) * kSwLd + ks * 16 + 8 * half);
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = *(const bf16x8*)(sP + ((2 * wave + j) * 32 + l31) * kSwLd + ks * 16 + 8 * half);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  // ---- acc[i][j][r]: channel 32 i + mfma32_row(r, lane), k = (2 wave + j) * 32 + (lane & 31)
  float* part = g.part + (long)blockIdx.x * 64 * 256;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        part[(32 * i + mfma32_row(r, lane)) * 256 + (2 * wave + j) * 32 + l31] = acc[i][j][r];
}

// dW[ch][(ty * 7 + tx) * 3 + c] += scale[ch]^2 * (part[0] + part[1] + ...)[ch][ty * 32 + tx * 4 + c], chunks ascending from 0
__global__ __launch_bounds__(256) void stem_wgrad_finish_kernel(const float* part, int chunks, const float* row_scale, float* dw, long dw_ld) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 64 * 147) return;
  const int ch = t / 147, kk = t - ch * 147;
  const int c = kk % 3, tap = kk / 3;
  const int ty = tap / 7, tx = tap - ty * 7;
  const float* src = part + ch * 256 + ty * 32 + tx * 4 + c;
  float s = 0.f;
  for (int i = 0; i < chunks; ++i) s += src[(long)i * 64 * 256];
  if (row_scale) s = __fmul_rn(__fmul_rn(row_scale[ch], row_scale[ch]), s);
  float* dst = dw + ch * dw_ld + kk;
  *dst = __fadd_rn(*dst, s);
}

static long stem_wgrad_chunks(int B, int Hc, int Wc) { return ((long)B * Hc * Wc + kSwChunk - 1) / kSwChunk; }

}  // namespace relnet

using namespace relnet;

// conv [B,H,W,C] (before bias), out / d_out [B,Ho,Wo,C] with Ho, Wo as relnet_stem_bias_relu_pool gives them for ksize 3, stride 2;
// dtype 0: fp32 (C % 4 == 0), 1: bf16 (C % 8 == 0); d_conv [B,H,W,C] in the same dtype, every element written.
extern "C" int relnet_stem_pool_bwd(const void* conv, const void* out, const void* d_out, void* d_conv, int B, int H, int W, int C,
                                    int dtype, void* stream) {
  RELNET_REQUIRE(conv && out && d_out && d_conv, "relnet_stem_pool_bwd: null operand");
  RELNET_REQUIRE(dtype == 0 || dtype == 1, "relnet_stem_pool_bwd: dtype is 0 (fp32) or 1 (bf16)");
  RELNET_REQUIRE(B > 0 && H >= 3 && W >= 3 && C > 0 && C % (dtype == 1 ? 8 : 4) == 0, "relnet_stem_pool_bwd: bad shape");
  RELNET_REQUIRE((((uintptr_t)conv | (uintptr_t)out | (uintptr_t)d_out | (uintptr_t)d_conv) & 15) == 0, "relnet_stem_pool_bwd: operands must be 16-byte aligned");
  int Ho = (H - 3 + 1) / 2 + 1, Wo = (W - 3 + 1) / 2 + 1;
  if ((Ho - 1) * 2 >= H) --Ho;               // last window must start inside the input
  if ((Wo - 1) * 2 >= W) --Wo;
  const long total = (long)B * H * W * (C / (dtype == 1 ? 8 : 4));
  const unsigned blocks = (unsigned)((total + 255) / 256);
  if (dtype == 1) {
    StemPoolBwdArgs<unsigned short> g{(const unsigned short*)conv, (const unsigned short*)out, (const unsigned short*)d_out,
                                      (unsigned short*)d_conv, B, H, W, C, Ho, Wo};
    stem_pool_bwd_kernel<unsigned short><<<blocks, 256, 0, (hipStream_t)stream>>>(g);
  } else {
    StemPoolBwdArgs<float> g{(const float*)conv, (const float*)out, (const float*)d_out, (float*)d_conv, B, H, W, C, Ho, Wo};
    stem_pool_bwd_kernel<float><<<blocks, 256, 0, (hipStream_t)stream>>>(g);
  }
  return check_launch("relnet_stem_pool_bwd");
}

extern "C" long relnet_stem_wgrad_workspace_bytes(int B, int Hc, int Wc) {
  if (B <= 0 || Hc <= 0 || Wc <= 0) return 0;
  return stem_wgrad_chunks(B, Hc, Wc) * 64 * 256 * (long)sizeof(float);
}

// packed [B,Hp,Wp,4] bf16 (relnet_stem_pack_input, pad 3), d_conv [B,Hc,Wc,64] bf16 dense; dw [64] rows of dw_ld floats, 147 written
// per row ((ty, tx, c) order); row_scale [64] or null.  The workspace needs no initialisation and is free again when the launches have run.
extern "C" int relnet_stem_wgrad(const void* packed, const void* d_conv, float* dw, long dw_ld, const float* row_scale, void* workspace,
                                 long workspace_bytes, int B, int Hp, int Wp, int Hc, int Wc, void* stream) {
  RELNET_REQUIRE(packed && d_conv && dw && workspace, "relnet_stem_wgrad: null operand");
  RELNET_REQUIRE(B > 0 && Hc > 0 && Wc > 0 && dw_ld >= 147, "relnet_stem_wgrad: bad shape");
  RELNET_REQUIRE(2 * (Hc - 1) + 8 <= Hp && 2 * (Wc - 1) + 8 <= Wp && Wp % 2 == 0, "relnet_stem_wgrad: padded image too small (Hp=%d Wp=%d)", Hp, Wp);
  RELNET_REQUIRE((((uintptr_t)packed | (uintptr_t)d_conv | (uintptr_t)workspace) & 15) == 0, "relnet_stem_wgrad: operands must be 16-byte aligned");
  const long chunks = stem_wgrad_chunks(B, Hc, Wc);
  RELNET_REQUIRE(workspace_bytes >= relnet_stem_wgrad_workspace_bytes(B, Hc, Wc), "relnet_stem_wgrad: the workspace holds %ld bytes, %ld needed",
                 workspace_bytes, relnet_stem_wgrad_workspace_bytes(B, Hc, Wc));
  RELNET_REQUIRE(chunks < (1L << 31), "relnet_stem_wgrad: too many pixels");
  StemWgradArgs g{(const unsigned short*)packed, (const unsigned short*)d_conv, (float*)workspace, (long)B * Hc * Wc, Hp, Wp, Hc, Wc};
  stem_wgrad_partial_kernel<<<(unsigned)chunks, 256, 0, (hipStream_t)stream>>>(g);
  stem_wgrad_finish_kernel<<<(64 * 147 + 255) / 256, 256, 0, (hipStream_t)stream>>>((const float*)workspace, (int)chunks, row_scale, dw, dw_ld);
  return check_launch("relnet_stem_wgrad");
}
