// Pairwise box geometry of the relation module (SYM_REL = relation_rcnn/symbols/
// resnet_v1_101_rcnn_attention_1024_pairwise_position_multi_head_16.py), shared by the forward kernel and the backward kernel that
// recomputes it: the geometry gradients are right only while both evaluate the same bits.
#pragma once
#include "common.h"

namespace relnet {

#pragma clang fp contract(off)
__device__ __forceinline__ void position_features(float4 bi, float4 bj, float (&p)[4]) {
  // bit-for-bit the fp32 op sequence of SYM_REL:59-77; log is correctly rounded (fp64
  // evaluation) because a 1-ulp log difference is amplified x100 before sin/cos.
  const float wi = bi.z - bi.x + 1.f, hi = bi.w - bi.y + 1.f;
  const float wj = bj.z - bj.x + 1.f, hj = bj.w - bj.y + 1.f;
  const float cxi = 0.5f * (bi.x + bi.z), cyi = 0.5f * (bi.y + bi.w);
  const float cxj = 0.5f * (bj.x + bj.z), cyj = 0.5f * (bj.y + bj.w);
  const float dx = fmaxf(fabsf((cxi - cxj) / wi), 1e-3f);
  const float dy = fmaxf(fabsf((cyi - cyj) / hi), 1e-3f);
  p[0] = (float)log((double)dx);
  p[1] = (float)log((double)dy);
  p[2] = (float)log((double)(wi / wj));
  p[3] = (float)log((double)(hi / hj));
}
#pragma clang fp contract(fast)

}  // namespace relnet
