// Wavefront and workgroup reductions shared by the kernel files.  Every reduction is a fixed tree: the same inputs give the
// same bits on every run.
#pragma once
#include "common.h"

namespace relnet {

// Butterfly sum / maximum over the 64 lanes; the result is the same in every lane.
template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// Workgroup sum of WAVES wavefronts in wave order, returned to every thread.  Contains one barrier; s holds WAVES values and
// belongs to this call alone (each sum of a kernel has its own array).
template <int WAVES, typename V>
__device__ __forceinline__ V block_sum(V v, V* s) {
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) s[threadIdx.x / kWave] = v;
  __syncthreads();
  V t = s[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) t += s[w];
  return t;
}

// Wave-wide maximum of a double without LDS traffic: four DPP steps inside each row of 16 lanes (quad_perm xor 1 / xor 2,
// row_half_mirror, row_mirror: the maximum is idempotent, mirrored partners are as good as a butterfly), then the four row values
// through v_readlane.  (__shfl_xor of a double is two ds_bpermute round trips per step; the per-pick arg-max chain of the
// class-NMS kernels is latency bound.)  The result is the same in every lane.
template <int CTRL> __device__ __forceinline__ double dpp_move_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double wave_max_dpp(double v) {
  v = fmax(v, dpp_move_f64<0xB1>(v));        // quad_perm [1,0,3,2]
  v = fmax(v, dpp_move_f64<0x4E>(v));        // quad_perm [2,3,0,1]
  v = fmax(v, dpp_move_f64<0x141>(v));       // row_half_mirror
  v = fmax(v, dpp_move_f64<0x140>(v));       // row_mirror
  return fmax(fmax(readlane_f64(v, 0), readlane_f64(v, 16)), fmax(readlane_f64(v, 32), readlane_f64(v, 48)));
}

// Wave-wide sum of an unsigned (same DPP pairing as wave_max_dpp: every step adds two disjoint groups).
__device__ __forceinline__ unsigned int wave_sum_dpp(unsigned int v) {
  v += (unsigned int)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, false);
  v += (unsigned int)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, false);
  v += (unsigned int)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, false);
  v += (unsigned int)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xf, 0xf, false);
  return (unsigned int)__builtin_amdgcn_readlane((int)v, 0) + (unsigned int)__builtin_amdgcn_readlane((int)v, 16) +
         (unsigned int)__builtin_amdgcn_readlane((int)v, 32) + (unsigned int)__builtin_amdgcn_readlane((int)v, 48);
}

#pragma clang fp contract(off)
// One wavefront: prob[c - first] = softmax(z)[c] for the classes c = first..C-1 (first = 1 drops the background column).
__device__ __forceinline__ void softmax_row(const float* z, float* prob, int C, int lane, int first) {
  float m = -INFINITY;
  for (int c = lane; c < C; c += kWave) m = fmaxf(m, z[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += kWave) s += expf(z[c] - m);
  s = wave_sum(s);
  for (int c = lane + first; c < C; c += kWave) prob[c - first] = expf(z[c] - m) / s;
}
#pragma clang fp contract(fast)

}  // namespace relnet
