// Test harness of include/relnet_operator_cxx.hpp's PSROIPooling classes: drives PSROIPoolingProp::InferShape + PSROIPoolingOp::Forward /
// Backward on caller-supplied device buffers (tests/test_operator_cxx_psroi.py loads it through ctypes).  Failed CHECKs come back as -1 +
// psroi_last_error().
#include <cstdio>
#include <memory>
#include <vector>

#include "relnet_operator_cxx.hpp"

using namespace relnet_op;

namespace {
char g_err[1024] = "";
}  // namespace

extern "C" const char* psroi_last_error() { return g_err; }

// data [N,C,H,W], rois [R,5], out / mapping [R,output_dim,pooled,pooled], dy like out or null (forward only), gdata like data,
// grois [R,5] or null; req_data / req_rois: OpReqType values (0 null, 1 write, 3 add); group 0 = pooled
extern "C" int psroi_pooling(const float* data, const float* rois, float* out, float* mapping, const float* dy, float* gdata, float* grois,
                             int N, int C, int H, int W, int R, int output_dim, int pooled, int group, float scale, int req_data,
                             int req_rois) {
  try {
    PSROIPoolingParam p;
    p.spatial_scale = scale; p.output_dim = output_dim; p.pooled_size = pooled; p.group_size = group;
    PSROIPoolingProp prop(p);
    if (prop.ListArguments() != std::vector<std::string>({"data", "rois"}) ||
        prop.ListOutputs() != std::vector<std::string>({"output", "mapping_channel"}) || prop.NumVisibleOutputs() != 1 ||
        prop.TypeString() != "_contrib_PSROIPooling" || prop.DeclareBackwardDependency({10}, {20, 21}, {30, 31}) != std::vector<int>({10, 21, 31}))
      return -3;
    std::vector<TShape> in = {{N, C, H, W}, {R, 5}};
    std::vector<TShape> outs;
    prop.InferShape(&in, &outs);
    if (outs.size() != 2 || outs[0] != TShape({R, output_dim, pooled, pooled}) || outs[1] != outs[0]) return -3;
    std::unique_ptr<PSROIPoolingOp> op(prop.CreateOperatorEx());
    OpContext ctx;
    std::vector<TBlob> in_data = {TBlob((void*)data, in[0]), TBlob((void*)rois, in[1])};
    std::vector<TBlob> out_data = {TBlob(out, outs[0]), TBlob(mapping, outs[1])};
    op->Forward(ctx, in_data, {kWriteTo, kWriteTo}, out_data);
    if (dy) {
      std::vector<TBlob> in_grad = {TBlob(gdata, in[0]), TBlob(grois, in[1])};
      op->Backward(ctx, {TBlob((void*)dy, outs[0])}, in_data, out_data, {(OpReqType)req_data, (OpReqType)req_rois}, in_grad);
    }
    if (hipDeviceSynchronize() != hipSuccess) return -4;
    return 0;
  } catch (const std::exception& e) {
    std::snprintf(g_err, sizeof(g_err), "%s", e.what());
    return -1;
  }
}
