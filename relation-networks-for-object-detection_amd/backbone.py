"""ResNet-101 conv1..conv5 + RPN head + conv_new_1 of the reference graph
(relation_rcnn/symbols/resnet_v1_101_rcnn_base.py:29-693, SYM_REL:249-250).

impl='hip' (bf16, the throughput path): every convolution, the 7x7 stem included, is a kernel of librelnet_hip.so over
NHWC activations -- the implicit-GEMM MFMA kernels of csrc/gemm.hip with bias / ReLU / shortcut fused into the epilogue,
the halo-resident 3x3 kernel and the block-boundary chain kernel of csrc/bottleneck.hip for res2; no library call.
impl='hip32' (float32 parity path, the default for dtype float32): the same graph on the exact-fp32 MFMA convolution kernel
(relnet_conv2d_nhwc_f32: an fmaf chain per output element) + relnet_maxpool_nhwc_f32 -- no library call either.
impl='miopen' runs the graph through torch.nn.functional.conv2d (kept for the A/B against the library).  What this module owns is the
graph itself: the Caffe-style ResNet (stride on the FIRST 1x1 of a stage, :99,103), conv5 dilated 2 with stride 1
(:632-633), ceil-mode pool1 (pooling_convention='full', :35-36) and the frozen BatchNorm (use_global_stats=True, eps=1e-5,
:32) folded into the preceding convolution at load time.
Parameter names are the reference's (`res4b7_branch2a_weight`, `bn4b7_branch2a_gamma`, ...).

The wiring is written once, as functions over a path's conv callable: `walk_units` (where conv4 and the stage ends are taken),
`bottleneck_unit`, `fpn_neck`, `rpn_head`.  `Backbone` runs them for inference; `TrunkTrain` runs them on a Trainer's weights, keeps the
activations, and holds the adjoint of each beside it.
"""
import math
import os
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import ops, train_ops as T

UNITS = (3, 4, 23, 3)
FILTERS = (256, 512, 1024, 2048)
EPS = 1e-5
PIXEL_MEANS = (103.06, 115.90, 123.15)      # network.PIXEL_MEANS (BGR) of every shipped experiment file


def unit_names(fpn=False):
    """[(stage, unit_name, in_ch, mid_ch, out_ch, stride, dilate, has_proj)] in graph order.  fpn: res5 has
    stride 2 and no dilation (symbols/resnet_v1_101_rcnn_fpn_..._learn_nms.py:707-720)."""
    out = []
    in_ch = 64
    for si, (n, oc) in enumerate(zip(UNITS, FILTERS)):
        stage = si + 2
        for u in range(n):
            if n <= 3 or stage == 2 or stage == 5:
                name = 'abc'[u]
            else:
                name = 'a' if u == 0 else 'b%d' % u
            stride = 2 if (u == 0 and (stage in (3, 4) or (fpn and stage == 5))) else 1
            dilate = 2 if (stage == 5 and not fpn) else 1
            out.append((stage, '%d%s' % (stage, name), in_ch, oc // 4, oc, stride, dilate, u == 0))
            in_ch = oc
    return out


def conv_bn_names():
    """[(conv_name, bn_name, out_ch, in_ch, k)] for every conv+BN pair of the backbone."""
    layers = [('conv1', 'bn_conv1', 64, 3, 7)]
    for stage, nm, ic, mc, oc, stride, dil, proj in unit_names():
        if proj:
            layers.append(('res%s_branch1' % nm, 'bn%s_branch1' % nm, oc, ic, 1))
        layers.append(('res%s_branch2a' % nm, 'bn%s_branch2a' % nm, mc, ic, 1))
        layers.append(('res%s_branch2b' % nm, 'bn%s_branch2b' % nm, mc, mc, 3))
        layers.append(('res%s_branch2c' % nm, 'bn%s_branch2c' % nm, oc, mc, 1))
    return layers


def init_params(seed=1, num_anchors=12, num_classes=81, num_reg_classes=2, generator=None, dcn_offset_std=0.0, fpn=False):
    """Random-init parameters of the relation test graph under the reference's names.
    New layers N(0, 0.01)/0 as init_weight (SYM_REL:327-362); the backbone has no pretrained
    weights offline: He-normal convs, BN gamma=1 (0.25 on the residual branch output so the
    34 residual adds keep activations O(1)), beta=0, mean=0, var=1."""
    g = generator or torch.Generator().manual_seed(seed)
    p = {}

    def nrm(std, *shape):
        return torch.randn(*shape, generator=g) * std

    for conv, bn, oc, ic, k in conv_bn_names():
        p[conv + '_weight'] = nrm(math.sqrt(2.0 / (ic * k * k)), oc, ic, k, k)
        p[bn + '_gamma'] = torch.full((oc,), 0.25 if conv.endswith('branch2c') else 1.0)
        p[bn + '_beta'] = torch.zeros(oc)
        p[bn + '_moving_mean'] = torch.zeros(oc)
        p[bn + '_moving_var'] = torch.ones(oc)
    p['rpn_conv_3x3_weight'] = nrm(0.01, 512, 1024, 3, 3); p['rpn_conv_3x3_bias'] = torch.zeros(512)
    p['rpn_cls_score_weight'] = nrm(0.01, 2 * num_anchors, 512, 1, 1); p['rpn_cls_score_bias'] = torch.zeros(2 * num_anchors)
    p['rpn_bbox_pred_weight'] = nrm(0.01, 4 * num_anchors, 512, 1, 1); p['rpn_bbox_pred_bias'] = torch.zeros(4 * num_anchors)
    p['conv_new_1_weight'] = nrm(0.01, 256, 2048, 1, 1); p['conv_new_1_bias'] = torch.zeros(256)
    p['fc_new_1_weight'] = nrm(0.01, 1024, 256 * 49); p['fc_new_1_bias'] = torch.zeros(1024)
    p['fc_new_2_weight'] = nrm(0.01, 1024, 1024); p['fc_new_2_bias'] = torch.zeros(1024)
    p['cls_score_weight'] = nrm(0.01, num_classes, 1024); p['cls_score_bias'] = torch.zeros(num_classes)
    p['bbox_pred_weight'] = nrm(0.01, 4 * num_reg_classes, 1024); p['bbox_pred_bias'] = torch.zeros(4 * num_reg_classes)
    for i in (1, 2):
        p['pair_pos_fc1_%d_weight' % i] = nrm(0.01, 16, 64); p['pair_pos_fc1_%d_bias' % i] = torch.zeros(16)
        p['query_%d_weight' % i] = nrm(0.01, 1024, 1024); p['query_%d_bias' % i] = torch.zeros(1024)
        p['key_%d_weight' % i] = nrm(0.01, 1024, 1024); p['key_%d_bias' % i] = torch.zeros(1024)
        p['linear_out_%d_weight' % i] = nrm(0.01, 1024, 1024, 1, 1); p['linear_out_%d_bias' % i] = torch.zeros(1024)
    # learn-NMS head, init_weight_nms (symbols/..._learn_nms.py:571-600): N(0,0.01) / 0, logit bias -3
    p['nms_rank_weight'] = nrm(0.01, 128, 1024); p['nms_rank_bias'] = torch.zeros(128)
    p['roi_feat_embedding_weight'] = nrm(0.01, 128, 1024); p['roi_feat_embedding_bias'] = torch.zeros(128)
    p['nms_pair_pos_fc1_1_weight'] = nrm(0.01, 16, 64); p['nms_pair_pos_fc1_1_bias'] = torch.zeros(16)
    p['nms_query_1_weight'] = nrm(0.01, 1024, 128); p['nms_query_1_bias'] = torch.zeros(1024)
    p['nms_key_1_weight'] = nrm(0.01, 1024, 128); p['nms_key_1_bias'] = torch.zeros(1024)
    p['nms_linear_out_1_weight'] = nrm(0.01, 128, 128, 1, 1); p['nms_linear_out_1_bias'] = torch.zeros(128)
    p['nms_logit_weight'] = nrm(0.01, 5, 128); p['nms_logit_bias'] = torch.full((5,), -3.0)
    # DCN configuration (symbols/resnet_v1_101_rcnn_dcn_..._learn_nms.py:700-746,1075).  The reference
    # initialises every offset predictor to ZERO (:1525-1535); `dcn_offset_std` > 0 gives non-trivial offsets
    # for tests / benches that have no trained weights.
    for u in 'abc':
        p['res5%s_branch2b_offset_weight' % u] = nrm(dcn_offset_std, 72, 512, 3, 3)
        p['res5%s_branch2b_offset_bias' % u] = torch.zeros(72)
    p['offset_weight'] = nrm(dcn_offset_std, 98, 256 * 49); p['offset_bias'] = torch.zeros(98)
    if fpn:     # symbols/...fpn...:1450-1470, 1508-1511: N(0, 0.01) / 0
        for lvl, cin in ((32, 2048), (16, 1024), (8, 512), (4, 256)):
            p['fpn_ft%d_1x1_weight' % lvl] = nrm(0.01, 256, cin, 1, 1); p['fpn_ft%d_1x1_bias' % lvl] = torch.zeros(256)
            p['fpn_ft%d_3x3_weight' % lvl] = nrm(0.01, 256, 256, 3, 3); p['fpn_ft%d_3x3_bias' % lvl] = torch.zeros(256)
        p['fpn_ft64_3x3_weight'] = nrm(0.01, 256, 256, 3, 3); p['fpn_ft64_3x3_bias'] = torch.zeros(256)
        p['roi_pool_fc1_weight'] = nrm(0.01, 1024, 256 * 49); p['roi_pool_fc1_bias'] = torch.zeros(1024)
        p['roi_pool_fc2_weight'] = nrm(0.01, 1024, 1024); p['roi_pool_fc2_bias'] = torch.zeros(1024)
    return p


def fold_bn(w, gamma, beta, mean, var, eps=EPS):
    """BatchNorm(use_global_stats=True, fix_gamma=False): y = (x-mean)/sqrt(var+eps)*gamma+beta."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return (w.double() * s.view(-1, 1, 1, 1)).float(), (beta.double() - mean.double() * s).float()


# ---- the graph, written once.  Every path (bf16 HIP kernels, exact-fp32 kernels, library convolutions, the training step) hands in its own
# conv(x, name, stride=1, pad=0, dil=1, relu=False, resid=None, out_dtype=None): layer `name` on x with bias (+ shortcut) (+ ReLU) in that
# path's layout and kernels.  What the functions below own is the wiring.

def walk_units(units, x, unit_fn, at_conv4=None):
    """x through `units` (rows of unit_names) by x = unit_fn(x, unit).  conv4 is the input of the first res5 unit -- at_conv4(conv4) is called
    there, before res5 is queued (the RPN branch forks at that point) -- and ends[s] the output of stage s, taken in front of the
    projection unit of stage s + 1 (the FPN laterals).  -> (output of the last unit, conv4, ends)"""
    conv4, ends = None, {}
    for unit in units:
        stage, proj = unit[0], unit[7]
        if stage == 5 and conv4 is None:
            conv4 = x
            if at_conv4 is not None:
                at_conv4(conv4)
        if proj and stage > 2:
            ends[stage - 1] = x
        x = unit_fn(x, unit)
    return x, conv4, ends


def bottleneck_unit(conv, x, unit, y_pre=None, sc=None, deform=None, expand=None, kept=None):
    """One bottleneck unit (resnet_v1_101_rcnn_base.py: branch1 | branch2a -> 2b -> 2c, + shortcut, ReLU).
    y_pre: the reduce output, when the previous unit's chain kernel already produced it.  sc: the shortcut operand, when the caller made it.
    deform(y1, name) -> (y2, off): the deformable 3x3 of a res5 unit with its offset convolution, in the caller's layout.
    expand(y2, sc) -> (x_next, reduce output of the NEXT unit | None), or None: a chain kernel in place of expand + shortcut + ReLU.
    kept: a list that receives y1, y2, off (what a training step keeps for the adjoint).  Without it each inner activation is released
    as soon as the next layer has read it, so the allocator hands its block to the layer after that.
    -> (x_next, next unit's reduce output | None)"""
    stage, nm, ic, mc, oc, stride, dil, proj = unit
    if sc is None:
        sc = conv(x, 'res%s_branch1' % nm, stride=stride) if proj else x
    y = y_pre if y_pre is not None else conv(x, 'res%s_branch2a' % nm, stride=stride, relu=True)
    if kept is not None:
        kept.append(y)
    if deform is not None and stage == 5:
        y, off = deform(y, 'res%s_branch2b' % nm)
    else:
        y, off = conv(y, 'res%s_branch2b' % nm, pad=dil, dil=dil, relu=True), None
    if kept is not None:
        kept.extend((y, off))
    del off
    out = expand(y, sc) if expand is not None else None
    if out is None:
        out = conv(y, 'res%s_branch2c' % nm, relu=True, resid=sc), None      # relu(bn(conv) + shortcut)
    return out


def fpn_neck(conv, upsample_add, conv5, ends):
    """Top-down pathway (symbols/..._fpn_...:804-840): 1x1 laterals, upsample_add(lateral, coarser top) = nearest 2x upsampling + sum,
    3x3 output convolutions.  -> (tops, feats), both {4, 8, 16, 32: map}."""
    tops = {32: conv(conv5, 'fpn_ft32_1x1')}
    for lvl, src in ((16, ends[4]), (8, ends[3]), (4, ends[2])):
        tops[lvl] = upsample_add(conv(src, 'fpn_ft%d_1x1' % lvl), tops[lvl * 2])
    return tops, {lvl: conv(tops[lvl], 'fpn_ft%d_3x3' % lvl, pad=1) for lvl in (4, 8, 16, 32)}


def rpn_head(conv, conv4):
    """-> (r = relu(rpn_conv_3x3(conv4)), the fused [.., 2A | 4A] score | delta map of the two 1x1 outputs, float32 on the HIP kernels)."""
    r = conv(conv4, 'rpn_conv_3x3', pad=1, relu=True)
    return r, conv(r, 'rpn_out', out_dtype=torch.float32)


class Backbone(object):
    """Folded, device-resident backbone + RPN head + conv_new_1.

    impl='hip' (bf16 only): every convolution except the 7x7/Cin=3 stem runs on the implicit-GEMM
    MFMA kernel of csrc/gemm.hip over NHWC activations, with bias + ReLU and the bottleneck's
    residual add + ReLU fused into the GEMM epilogue (the library path spends as long in separate
    bias / add / clamp passes as in the convolutions themselves).  impl='miopen' keeps every conv
    in torch.nn.functional.conv2d (used for the float32 parity path)."""

    def __init__(self, params, dtype=torch.bfloat16, device='cuda', channels_last=True, impl=None, stem='hip', dcn=False,
                 fpn=False, chain=True, frozen_only=False, pixel_means=PIXEL_MEANS):
        """pixel_means: network.PIXEL_MEANS (BGR), subtracted on the device from uint8 [B,H,W,3] BGR HWC input (see `forward`).
        frozen_only: pack conv1 + res2 only (what `forward_res2` runs): the part the training step never updates
        (cfgs/*.yaml FIXED_PARAMS) -- the Trainer keeps res3 .. heads in its own flat buffers, a second bf16 copy of them here would
        be a few hundred MB of stale weights."""
        self.dtype, self.device, self.dcn, self.fpn = dtype, device, dcn, fpn
        self.frozen_only = frozen_only
        self.pixel_means = tuple(float(v) for v in pixel_means)
        self.use_chain = chain
        env = os.environ.get('RELNET_STAGE_SPLIT')        # A/B knob: '4:2,5:4' = stage:sub-batches ('0' / unset: no split)
        if env not in (None, '', '0'):
            self.stage_split = {int(a): int(b) for a, b in (kv.split(':') for kv in env.split(','))}
        if os.environ.get('RELNET_INPLACE_EXPAND') is not None:
            self.inplace_expand = os.environ['RELNET_INPLACE_EXPAND'] not in ('', '0')
        if os.environ.get('RELNET_QUARTER_UNITS') is not None:
            self.quarter_units = os.environ['RELNET_QUARTER_UNITS'] not in ('', '0')
        self.impl = impl or ('hip' if dtype == torch.bfloat16 else ('hip32' if dtype == torch.float32 and torch.device(device).type == 'cuda' else 'miopen'))
        if self.impl == 'hip' and torch.device(device).type == 'cuda':
            ops.asm_selfcheck()          # tile 19 (AGPR accumulators across asm statements) against the compiler-scheduled tile, once per process
        self.stem = stem
        assert self.impl in ('hip', 'hip32', 'miopen') and (self.impl != 'hip' or dtype == torch.bfloat16) and (self.impl != 'hip32' or dtype == torch.float32)
        self.mf = torch.channels_last if channels_last else torch.contiguous_format
        self.w = {}
        self.wp = {}
        self.wf = {}          # name -> fragment-order weight copy (panel kernel)
        self.b32 = {}
        self.wp32 = {}        # impl 'hip32': name -> ([Cout, k*k*Cin] fp32 packed weight, fp32 bias, k)
        for conv, bn, oc, ic, k in conv_bn_names():
            if frozen_only and not conv.startswith(('conv1', 'res2')):
                continue
            w, b = fold_bn(params[conv + '_weight'], params[bn + '_gamma'], params[bn + '_beta'],
                           params[bn + '_moving_mean'], params[bn + '_moving_var'])
            self._put(conv, w, b)
        if frozen_only:
            pass
        elif fpn:     # FPN neck instead of the RPN head / conv_new_1 (HAS_RPN: false in the FPN relation configs)
            for lvl in (32, 16, 8, 4):
                for k in ('1x1', '3x3'):
                    name = 'fpn_ft%d_%s' % (lvl, k)
                    self._put(name, params[name + '_weight'], params[name + '_bias'])
        else:
            for name in ('rpn_conv_3x3', 'rpn_cls_score', 'rpn_bbox_pred', 'conv_new_1'):
                self._put(name, params[name + '_weight'], params[name + '_bias'])
            # both 1x1 RPN outputs in one convolution: 24 score + 48 delta channels
            self._put('rpn_out', torch.cat([params['rpn_cls_score_weight'], params['rpn_bbox_pred_weight']], 0),
                      torch.cat([params['rpn_cls_score_bias'], params['rpn_bbox_pred_bias']], 0))
        self.units = [u for u in unit_names(fpn) if not frozen_only or u[0] == 2]
        self.wp_dcn = {}
        if dcn and not frozen_only:     # res5{a,b,c}_branch2b become DeformableConvolution(num_deformable_group=4) fed by a 72-channel offset conv
            for u in 'abc':
                name = 'res5%s_branch2b' % u
                self._put(name + '_offset', params[name + '_offset_weight'], params[name + '_offset_bias'])
                w, b = fold_bn(params[name + '_weight'], params['bn5%s_branch2b_gamma' % u], params['bn5%s_branch2b_beta' % u],
                               params['bn5%s_branch2b_moving_mean' % u], params['bn5%s_branch2b_moving_var' % u])
                self.wp_dcn[name] = (ops.pack_conv_weight(w, self.dtype, self.device), b.to(self.device, torch.float32).contiguous())
        if self.impl == 'hip':
            w1, b1 = fold_bn(params['conv1_weight'], params['bn_conv1_gamma'], params['bn_conv1_beta'],
                             params['bn_conv1_moving_mean'], params['bn_conv1_moving_var'])
            self.w_stem = ops.pack_stem_weight(w1, self.dtype, self.device)
            self.zero_bias64 = torch.zeros(64, device=self.device, dtype=torch.float32)
        # block boundaries inside a stage (identity shortcut, stride 1) of the HBM-bound stages: expand + shortcut + ReLU of
        # unit u and reduce + ReLU of unit u+1 as one pixel-wise kernel (ops.bottleneck_chain); unit -> its operands
        self.chain, self.halo3, self.chain_proj = {}, {}, {}
        if self.impl == 'hip' and chain:
            # (A/B knob: RELNET_CHAIN_REDUCE256=0 keeps res4's reduce layers as their own launches, the round-3 form)
            reduce_mids = tuple(m for m in ops.CHAIN_MIDS if m != 256 or os.environ.get('RELNET_CHAIN_REDUCE256', '1') != '0')
            for (st, nm, ic, mc, oc, stride, dil, proj), nxt in zip(self.units, self.units[1:] + [None]):
                if nxt is not None and nxt[0] == st and not nxt[7] and mc in reduce_mids:
                    w3, b3, _ = self.wp['res%s_branch2c' % nm]
                    w1n, b1n, _ = self.wp['res%s_branch2a' % nxt[1]]
                    self.chain[nm] = (ops.pack_w_frag(w3), ops.pack_chain_w1(w1n), b3, b1n)
                elif mc in ops.CHAIN_EXPAND_MIDS:   # last unit of a stage, and every res4 unit: the kernel without the second product
                    w3, b3, _ = self.wp['res%s_branch2c' % nm]
                    self.chain[nm] = (ops.pack_w_frag(w3), None, b3, None)
            # first unit of res2: its stride-1 projection shortcut rides in the expand product (ops.bottleneck_chain_proj)
            for (st, nm, ic, mc, oc, stride, dil, proj) in self.units:
                if proj and stride == 1 and mc == 64 and ic == 64 and nm in self.chain:
                    w3f, w1f, b3, b1n = self.chain[nm]
                    wp_, bp_, _ = self.wp['res%s_branch1' % nm]
                    self.chain_proj[nm] = (w3f, ops.pack_w_frag(wp_), w1f, (b3 + bp_).contiguous(), b1n)
            # 64-channel 3x3 convolutions (res2 branch2b): halo tile resident in LDS instead of one LDS fill per tap
            for st, nm, ic, mc, oc, stride, dil, proj in self.units:
                if mc in ops.HALO3_CHANNELS and dil == 1 and not (self.dcn and st == 5):
                    w, b, _ = self.wp['res%s_branch2b' % nm]
                    self.halo3['res%s_branch2b' % nm] = (ops.pack_w_frag(w, panel_only=False), b)

    def _put(self, name, w, b):
        self.w[name] = (w.to(self.device, self.dtype).contiguous(memory_format=self.mf),
                        b.to(self.device, self.dtype))
        if self.impl == 'hip':
            self.b32[name] = b.to(self.device, torch.float32).contiguous()
        if self.impl == 'hip32':
            if w.shape[1] % 16:             # the 3-channel stem: zero input channels up to 16 (the kernel's k granularity)
                wz = torch.zeros((w.shape[0], (w.shape[1] + 15) // 16 * 16) + tuple(w.shape[2:]), dtype=w.dtype)
                wz[:, :w.shape[1]] = w
                w = wz
            self.wp32[name] = (ops.pack_conv_weight(w, torch.float32, self.device), b.to(self.device, torch.float32).contiguous(), int(w.shape[2]))
        if self.impl == 'hip' and w.shape[1] % 64 == 0:
            self.wp[name] = (ops.pack_conv_weight(w, self.dtype, self.device),
                             b.to(self.device, torch.float32).contiguous(), int(w.shape[2]))
            # 256-deep expand convolutions (res4 branch2c, 23 per step): a second copy of the weights in MFMA-fragment
            # order lets relnet_conv2d_nhwc_wf pick the panel kernel (A resident in LDS, W streamed through registers)
            if self.dtype == torch.bfloat16 and tuple(w.shape[1:]) == (256, 1, 1) and w.shape[0] % 256 == 0 \
                    and name.endswith('_branch2c'):
                self.wf[name] = ops.pack_w_frag(self.wp[name][0])

    def _hconv(self, x, name, stride=1, pad=0, dil=1, relu=False, resid=None, out_dtype=None):
        if name in self.halo3 and stride == 1:      # 64-channel 3x3 (res2 branch2b): the halo-resident kernel
            return ops.conv3x3_halo(x.contiguous(), *self.halo3[name], relu=relu)
        w, b, k = self.wp[name]
        return ops.conv2d_nhwc(x, w, b, ksize=k, stride=stride, pad=pad, dil=dil, relu=relu, resid=resid,
                               out_dtype=out_dtype, w_frag=self.wf.get(name))

    def _float_image(self, data, im_info, dtype):
        """uint8 [B,H,W,3] BGR HWC -> [B,3,H,W] `dtype` RGB NCHW with the means subtracted inside each image's extent
        (ops.image_transform_u8: what dataset/image.py:transform + tensor_vstack give); NCHW float input is returned as it is."""
        if data.dtype != torch.uint8:
            return data
        return ops.image_transform_u8(data, self.pixel_means, im_info, dtype=dtype)

    def forward_res2(self, data, im_info=None):
        """Stem + res2 only (the part the reference freezes in training: cfgs/*.yaml FIXED_PARAMS conv1 / res2): raw NCHW image ->
        res2c output, NHWC bf16, on the inference kernels (fused stem, halo 3x3, chain kernels incl. res2a's in-kernel projection).
        data and im_info as in `forward`."""
        if self.impl == 'hip32':           # float32 parity path (frozen_only backbones return the res2c map)
            assert self.frozen_only
            return self._forward_hip32(self._float_image(data, im_info, torch.float32))
        x = ops.stem_fused(data, self.w_stem, self.b32['conv1'], im_info, self.pixel_means)
        y_next = None
        self.last_chain_units = []
        for unit in self.units:
            if unit[0] != 2:
                break
            x, y_next = self._unit_hip(x, unit, y_next)
        return x

    def forward_stem(self, data, im_info=None):
        """conv1 + bn_conv1 + ReLU + pool1 only (a training step whose res2 is trainable above a fixed conv1): the fused stem, or its
        float32 twin -> pooled NHWC map."""
        if self.impl == 'hip32':
            data = self._float_image(data, im_info, torch.float32)
            B, Cin, H, W = data.shape
            x = torch.zeros((B, H, W, 16), device=data.device, dtype=torch.float32)
            x[..., :Cin] = data.permute(0, 2, 3, 1)
            return ops.maxpool_nhwc_f32(self._c32(x, 'conv1', stride=2, pad=3, relu=True), 3, 2)
        return ops.stem_fused(data, self.w_stem, self.b32['conv1'], im_info, self.pixel_means)

    def _forward_hip(self, data, rpn_hook=None, im_info=None):
        if self.stem == 'hip':
            # conv1 7x7/2 + bias + ReLU + pool1 in ONE kernel, raw NCHW (or uint8 HWC) image -> pooled NHWC map (no conv map in HBM)
            x = ops.stem_fused(data, self.w_stem, self.b32['conv1'], im_info, self.pixel_means)
        elif self.stem == 'hip3':
            # the three-launch form: repack to padded NHWC4, 7x7/2 conv + bias + ReLU on the MFMA kernel, then pool1
            x = ops.stem_conv7(self._float_image(data, im_info, torch.float32), self.w_stem, self.b32['conv1'], relu=True)
            x = ops.stem_bias_relu_pool(x, self.zero_bias64)
        else:
            # library 7x7 convolution (no bias), then ONE kernel for bias + ReLU + pool1
            x = self._float_image(data, im_info, torch.float32).to(self.dtype).contiguous(memory_format=self.mf)
            x = F.conv2d(x, self.w['conv1'][0], None, stride=2, padding=3)
            x = ops.stem_bias_relu_pool(x.permute(0, 2, 3, 1), self.b32['conv1'])
        side, hooked = None, None
        self.last_chain_units, self.last_side_stream, self.last_stage_split = [], False, {}      # what actually ran (reported by oracle/parity.py)
        self.last_quarter_units = []
        after = dict(zip(self.units, self.units[1:]))
        y_next = None
        compact = False                   # x is the even-pixel quarter of the previous stage's output (its last unit ran in the quarter form)
        split = None                      # the stage that ran whole, in sub-batches, at its first unit

        def fork(conv4):                  # RPN head + hook next to res5
            nonlocal side, hooked
            if rpn_hook is None or self.fpn:
                return
            main = torch.cuda.current_stream()
            side = self._side_stream()
            self.last_side_stream = True
            side.wait_stream(main)
            with torch.cuda.stream(side):
                hooked = self._rpn_head(conv4)
                hooked = hooked + (rpn_hook(hooked[0], hooked[1]),)

        def unit_fn(x, unit):             # which kernels run a unit: stage split, quarter form, in-place expand
            nonlocal y_next, compact, split
            stage, proj = unit[0], unit[7]
            if stage == split:
                return x
            nsplit = self._stage_split(stage, x, unit) if proj else 1
            if nsplit > 1:
                # Infinity-Cache-sized sub-batches (see _stage_split): all units of the stage on images [lo, hi), then the next range
                split = stage
                return self._run_stage_split(x, [u for u in self.units if u[0] == stage], nsplit)
            quarter = self._quarter_ok(x, unit, after.get(unit))
            x, y_next = self._unit_hip(x, unit, y_next, inplace=self.inplace_expand, quarter=quarter, subsampled=compact)
            compact = quarter
            return x

        conv5, conv4, ends = walk_units(self.units, x, unit_fn, fork)
        return self._outputs(self._hconv, conv5, conv4, ends, lambda t: t.permute(0, 3, 1, 2), ops.upsample2x_add_, hooked, side)

    def _outputs(self, conv, conv5, conv4, ends, nchw, upsample_add, hooked=None, side=None):
        """What hangs off the trunk, as `forward`'s dictionary: the FPN neck, or conv_new_1 + the RPN head (`hooked`: the head ran on the
        side stream with the caller's hook behind it).  nchw: this path's activation layout -> logical NCHW."""
        if self.fpn:
            _, feats = fpn_neck(conv, upsample_add, conv5, ends)
            out = {'fpn_ft%d' % lvl: nchw(feats[lvl]) for lvl in (4, 8, 16, 32)}
            out.update(conv4=nchw(conv4), conv5=nchw(conv5))
            return out
        feat = conv(conv5, 'conv_new_1', relu=True)
        out = dict(conv4=nchw(conv4), conv5=nchw(conv5), conv_new_1_relu=nchw(feat))
        if hooked is not None:
            torch.cuda.current_stream().wait_stream(side)      # join
            out.update(rpn_cls_score=hooked[0], rpn_bbox_pred=hooked[1], rpn_hook=hooked[2])
        else:
            out['rpn_cls_score'], out['rpn_bbox_pred'] = self._rpn_head(conv4, conv, nchw)
        return out

    #: stage -> sub-batches (default: none).  Measured in round 4 and NOT adopted: running the 23 res4 units on two 27-image halves so
    #: that the 1024-channel activation (265 MB at 54 images, just over the 256 MB Infinity Cache) stays cache-resident.  The
    #: memory-side cache does keep a rewritten buffer (in-place elementwise pass: 7.0-7.3 TB/s up to 256 MB against 6.0 TB/s
    #: beyond), but that is only +20 % on the HBM rate, and half-size launches lose more at their seams: 21.8 / 22.05 ms unsplit
    #: against 22.2 / 22.4 ms split on the same box (tools/llc_probe.py, tools/scripts/r04_ab_split.sh).  Kept as an A/B knob:
    #: RELNET_STAGE_SPLIT=4:2.
    stage_split = None
    #: x_next written over the shortcut operand by the expand kernels (inference only: a unit's input is destroyed once its reduce
    #: convolution has read it).  Halves the activation footprint of a stage; RELNET_INPLACE_EXPAND=0 for the A/B.
    inplace_expand = True

    #: the last unit of res2 / res3 computed at the even (y, x) pixels only (non-FPN graphs): nothing but the stride-2 1x1 layers of
    #: res3a / res4a reads its output, so its 3x3 layer runs at stride 2 and its expand kernel gathers the shortcut
    #: (ops.conv3x3_halo_s2 / conv2d_nhwc(stride=2), ops.bottleneck_chain_s2); the next unit then runs at stride 1 on the compact map.
    #: Same bits as the dense form at the pixels that are read.  RELNET_QUARTER_UNITS=0 for the A/B.
    quarter_units = True

    def _quarter_ok(self, x, unit, nxt):
        """Does `unit` (about to run on x) run in the quarter form?  Its successor must be a stride-2 projection unit of the next stage and
        the only reader of its output (no FPN laterals), neither stage may be split, and the gather kernel must be worthwhile at the
        COMPACT pixel count."""
        stage, nm, ic, mc, oc, stride, dil, proj = unit
        if not self.quarter_units or self.fpn or nxt is None or nxt[0] != stage + 1 or nxt[5] != 2 or not nxt[7]:
            return False
        ch = self.chain.get(nm)
        if ch is None or ch[1] is not None or mc not in ops.CHAIN_S2_MIDS or proj or dil != 1 or (self.dcn and stage == 5):
            return False
        if mc in ops.HALO3_CHANNELS and ('res%s_branch2b' % nm) not in self.halo3:
            return False
        if self.stage_split and (self._stage_split(stage, x, unit) > 1 or self._stage_split(nxt[0], x, nxt) > 1):
            return False
        B, H, W, C = x.shape
        return C == oc and x.numel() * 2 < (1 << 32) and ops.chain_worthwhile(B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1), mc)

    def _stage_split(self, stage, x, unit):
        return int(self.stage_split.get(stage, 1)) if self.stage_split else 1

    def _run_stage_split(self, x, stage_units, nsplit):
        B = x.shape[0]
        stage = stage_units[0][0]
        st, nm, ic, mc, oc, stride, dil, proj = stage_units[0]
        Ho, Wo = (x.shape[1] - 1) // stride + 1, (x.shape[2] - 1) // stride + 1
        out = torch.empty((B, Ho, Wo, oc), device=x.device, dtype=x.dtype)
        bounds = [(B * i) // nsplit for i in range(nsplit + 1)]
        self.last_stage_split[stage] = [hi - lo for lo, hi in zip(bounds, bounds[1:])]
        for lo, hi in zip(bounds, bounds[1:]):
            xs, ys = x[lo:hi], None
            for unit in stage_units:
                xs, ys = self._unit_hip(xs, unit, ys, sc_out=out[lo:hi] if unit[7] else None, inplace=self.inplace_expand, force_chain=True)
            if xs.data_ptr() != out[lo:hi].data_ptr():
                out[lo:hi].copy_(xs)
        return out

    def _unit_hip(self, x, unit, y_pre=None, sc_out=None, inplace=False, force_chain=False, quarter=False, subsampled=False):
        """One bottleneck unit (resnet_v1_101_rcnn_base.py: branch1 | branch2a -> 2b -> 2c, + shortcut, ReLU) on the HIP kernels.
        y_pre: this unit's reduce output if the previous unit's chain kernel already produced it.  sc_out: where the projection
        shortcut of a first unit is written.  inplace: the expand kernel may write x_next over its shortcut operand.
        quarter: only the even (y, x) pixels of x_next are produced, as a compact map (see `quarter_units`).  subsampled: x is such a
        compact map, i.e. this unit's stride 2 has already been applied.
        -> (x_next, reduce output of the NEXT unit | None)"""
        stage, nm, ic, mc, oc, stride, dil, proj = unit
        if subsampled:
            assert stride == 2 and proj
            stride = 1
        if quarter:
            y = y_pre if y_pre is not None else self._hconv(x, 'res%s_branch2a' % nm, relu=True)
            if ('res%s_branch2b' % nm) in self.halo3:
                y = ops.conv3x3_halo_s2(y.contiguous(), *self.halo3['res%s_branch2b' % nm], relu=True)
            else:
                y = self._hconv(y, 'res%s_branch2b' % nm, stride=2, pad=1, relu=True)
            w3f, _, b3, _ = self.chain[nm]
            if nm not in self.last_chain_units:
                self.last_chain_units.append(nm)
            self.last_quarter_units.append(nm)
            return ops.bottleneck_chain_s2(y, x.contiguous(), w3f, b3), None
        fuse_proj = (nm in self.chain_proj and sc_out is None and x.is_contiguous()
                     and (force_chain or ops.chain_worthwhile(x.numel() // x.shape[-1], mc)))
        sc = None
        if fuse_proj:
            sc = x                   # res2a: the expand kernel projects its shortcut operand itself
        elif proj and sc_out is not None:
            w, b, k = self.wp['res%s_branch1' % nm]
            sc = ops.conv2d_nhwc(x, w, b, ksize=k, stride=stride, out=sc_out)

        def chain(y, sc):            # expand + shortcut + ReLU and the next unit's reduce + ReLU in one pixel-wise kernel
            ch = self.chain.get(nm)
            if not fuse_proj and (ch is None or not (force_chain or ops.chain_worthwhile(y.numel() // y.shape[-1], y.shape[-1]))):
                return None          # small maps (B = 1, late stages at small B): the tiled convolution kernels fill the GPU better
            if nm not in self.last_chain_units:
                self.last_chain_units.append(nm)  # (a split stage, `inplace`, is only entered when every CU gets a 256-pixel set)
            if fuse_proj:
                return ops.bottleneck_chain_proj(y, x, *self.chain_proj[nm])
            return ops.bottleneck_chain(y, sc.contiguous(), *ch, inplace=inplace and sc.is_contiguous())
        return bottleneck_unit(self._hconv, x, unit[:5] + (stride,) + unit[6:], y_pre, sc, self._deform_nhwc(self._hconv), chain)

    def _rpn_head(self, conv4, conv=None, nchw=lambda t: t.permute(0, 3, 1, 2)):
        rpn = nchw(rpn_head(conv or self._hconv, conv4)[1])
        na2 = self.w['rpn_cls_score'][0].shape[0]
        return rpn[:, :na2], rpn[:, na2:]

    def _side_stream(self):
        if getattr(self, '_side', None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    def _deform_2b(self, y, name, offset):
        """DeformableConvolution(kernel 3x3, pad 2, dilate 2, num_deformable_group 4, no_bias) + BN + ReLU
        (SYM_DCN_RELNMS:700-707); y / offset logical NCHW."""
        w, b = self.wp_dcn[name]
        return ops.deformable_conv(y, offset, w, b, 3, 1, 2, 2, 4, relu=True)

    def _deform_nhwc(self, conv):
        """bottleneck_unit's `deform` for the NHWC paths (None without dcn): offset convolution on `conv`, then `_deform_2b`."""
        if not self.dcn:
            return None

        def deform(y, name):
            off = conv(y, name + '_offset', pad=2, dil=2, out_dtype=torch.float32)
            return self._deform_2b(y.permute(0, 3, 1, 2), name, off.permute(0, 3, 1, 2)).permute(0, 2, 3, 1), off
        return deform

    def _conv(self, x, name, stride=1, pad=0, dil=1, relu=False, resid=None, out_dtype=None):
        """(out_dtype is the HIP kernels' argument: the library path and the float32 path keep their own type)"""
        w, b = self.w[name]
        y = F.conv2d(x, w, b, stride=stride, padding=pad, dilation=dil)
        if resid is not None:
            y.add_(resid)
        return F.relu_(y) if relu else y

    def _c32(self, x, name, stride=1, pad=0, dil=1, relu=False, resid=None, out_dtype=None):
        w, b, k = self.wp32[name]
        return ops.conv2d_nhwc_f32(x, w, b, ksize=k, stride=stride, pad=pad, dil=dil, relu=relu, resid=resid)

    def _forward_hip32(self, data):
        """The float32 parity path on this repository's own kernels: every convolution on relnet_conv2d_nhwc_f32 (exact-fp32 MFMA, bias /
        shortcut / ReLU in the epilogue), pool1 on relnet_maxpool_nhwc_f32, NHWC float32 activations."""
        B, Cin, H, W = data.shape
        x = torch.zeros((B, H, W, 16), device=data.device, dtype=torch.float32)       # NHWC, channels zero-padded 3 -> 16
        x[..., :Cin] = data.permute(0, 2, 3, 1)
        x = self._c32(x, 'conv1', stride=2, pad=3, relu=True)
        x = ops.maxpool_nhwc_f32(x, 3, 2)
        deform = self._deform_nhwc(self._c32)
        conv5, conv4, ends = walk_units(self.units, x, lambda x, unit: bottleneck_unit(self._c32, x, unit, deform=deform)[0])
        if self.frozen_only:
            return conv5
        return self._outputs(self._c32, conv5, conv4, ends, lambda t: t.permute(0, 3, 1, 2), ops.upsample2x_add_)

    def forward(self, data, rpn_hook=None, im_info=None):
        """data [B,3,H,W] float NCHW (RGB, means subtracted: dataset/image.py:get_image), or [B,H,W,3] uint8 BGR HWC as decoded /
        resized (ops.resize_u8): the means (`pixel_means`) are then subtracted on the device inside each image's extent im_info[:, :2]
        ([B,3] fp32 device; None = the whole canvas) and the rest reads 0, which is the reference's padding rule -- the fused stem
        reads the uint8 canvas itself (relnet_stem_fused_u8), every other path converts it first (relnet_image_transform_u8).
        -> dict(conv4, conv5, conv_new_1_relu, rpn_cls_score, rpn_bbox_pred)
        (logical NCHW tensors; channels-last memory).

        rpn_hook (impl 'hip'): callable(rpn_cls_score, rpn_bbox_pred) -> anything, e.g. the proposal operator.  The RPN head
        and the hook then run on a SIDE stream as soon as conv4 exists, concurrently with res5 / conv_new_1 on the caller's
        stream (the proposal kernels are latency bound and occupy ~54 workgroups; res5 fills the rest of the GPU); the two
        streams join before this function returns and the hook's result is returned under the key 'rpn_hook'."""
        if self.impl == 'hip':
            return self._forward_hip(data, rpn_hook, im_info)
        if self.impl == 'hip32':
            return self._forward_hip32(self._float_image(data, im_info, torch.float32))
        x = self._float_image(data, im_info, torch.float32).to(self.dtype).contiguous(memory_format=self.mf)
        x = self._conv(x, 'conv1', stride=2, pad=3, relu=True)
        x = F.max_pool2d(x, kernel_size=3, stride=2, padding=0, ceil_mode=True)

        def deform(y, name):
            off = self._conv(y, name + '_offset', pad=2, dil=2).float()
            return self._deform_2b(y, name, off).contiguous(memory_format=self.mf), off
        conv5, conv4, ends = walk_units(self.units, x, lambda x, unit: bottleneck_unit(self._conv, x, unit, deform=deform if self.dcn else None)[0])
        return self._outputs(self._conv, conv5, conv4, ends, lambda t: t, lambda lateral, top: F.interpolate(top, scale_factor=2, mode='nearest') + lateral)


# workgroups of the RPN head's grouped weight-gradient launch on the side stream: a quarter of the chip, the head's kernels beside it keep
# theirs (same box, 8 images: 16.99 ms per step with these products in the heads bucket's launch on the main stream, 16.92 on 32 workgroups,
# 16.87 - 16.89 on 64, 16.99 on 128)
RPN_WGRAD_WORKGROUPS = 64

#: what the training forward keeps of one unit for its adjoint (off: (offset map, sampled column matrix) of a deformable unit | None)
SavedUnit = namedtuple('SavedUnit', 'stage nm stride dil proj x y1 y2 out off')
#: ... and of a trainable stem: image = what conv1's weight gradient reads (the packed NHWC4 bf16 image; the float NCHW image for the float32
#: trunk), conv = the conv1 map before bias, out = relu(pool1(conv) + bias)
SavedStem = namedtuple('SavedStem', 'image conv out')


class TrunkTrain(object):
    """res3 .. res5, the FPN neck and the RPN head convolutions of a training step, each with its adjoint beside it, on a Trainer's
    parameters (as relation.BoxHeadTrain is for the box head).  The forwards are the functions above on the trainer's `_conv`; the trainer
    owns the parameters, their relayout entries, the gradient buffers and the queues, reached through w / wt / b / conv_bias / bn_scale,
    _wg / _bg / _add_wgrad / _add_bgrad and _bucket_ready, and it keeps chain_units, mask_epilogue, _fragpack and _relayout: all of them
    are read when a method runs, so in-place optimizer updates and a flipped switch are seen without a rebuild."""

    def __init__(self, trainer):
        """Registers res3 .. res5's block boundaries for the inference chain kernels (csrc/bottleneck.hip): expand + shortcut + ReLU of unit u
        and reduce + ReLU of unit u + 1 in one launch.  They read the weights in MFMA-fragment order; the trained weights change every
        step, so ONE grouped launch per step (trainer._fragpack, an ops.FragRepack) rewrites those copies next to the data-gradient
        layouts.  trainer.chain_units: unit -> (has_next_reduce, next unit).  (The float32 trunk keeps the per-layer convolution launches.)"""
        t = self.t = trainer
        t._fragpack, t.chain_units = ops.FragRepack(t.device), {}
        if not t.trunk_fp32:
            trainable = [u for u in t.units if u[0] >= 3]
            for (st, nm, ic, mc, oc, stride, dil, proj), nxt in zip(trainable, trainable[1:] + [None]):
                if t.cfg.dcn and st == 5:
                    continue
                with_reduce = nxt is not None and nxt[0] == st and not nxt[7] and mc in ops.CHAIN_MIDS
                if not with_reduce and mc not in ops.CHAIN_EXPAND_MIDS:
                    continue
                t._fragpack.add('w3:' + nm, t.w('res%s_branch2c' % nm), 0)
                if with_reduce:
                    t._fragpack.add('w1:' + nxt[1], t.w('res%s_branch2a' % nxt[1]), 1)
                t.chain_units[nm] = (with_reduce, nxt[1] if with_reduce else None)
            t._fragpack.build()

    def _dgrad_w(self, name, cout):
        """[Cout, 9*Cin] packed forward weights -> [Cin, 9*Cout] tap-flipped data-gradient weights."""
        wt = self.t.wt(name)
        if wt is not None:
            return wt
        w = self.t.w(name)
        cin = w.shape[1] // 9
        return w.view(cout, 3, 3, cin).flip(1, 2).permute(3, 1, 2, 0).reshape(cin, 9 * cout).contiguous()

    # ---- res3 .. res5 ----------------------------------------------------------------------------------------
    def forward(self, data, at_conv4=None, im_info=None):
        """Frozen stem + res2 (or, where network.FIXED_PARAMS leaves them trainable, res2 / conv1 on the trainer's weights like the rest), then
        res3..res5 keeping every ReLU output.  Returns (conv5, conv4, saved units, stage ends).
        at_conv4(conv4): called once conv4 exists, before res5 is queued (the RPN branch forks there).  data: float NCHW or uint8
        [B,H,W,3] BGR HWC (Backbone.forward; im_info gives each image's extent)."""
        t = self.t
        saved = []
        if t.stem_trainable:       # conv1 .. res5 on the trainer's weights; saved[0] is the stem's SavedStem
            x = self._stem_forward(data, im_info, saved)
        elif t.res2_trainable:     # fixed conv1 on the fused stem, res2 .. res5 on the trainer's weights
            x = t._frozen_backbone.forward_stem(data, im_info)
        else:
            x = t._frozen_backbone.forward_res2(data, im_info)      # (float32 NHWC for the float32 trunk: Backbone impl 'hip32')
        y_pre = None               # reduce output of the coming unit when the previous unit's chain kernel already produced it

        def deform(y1, nb):        # 72-channel offset conv -> DeformableConvolution(num_deformable_group=4) + BN + ReLU
            off = t._conv(y1, nb + '_offset', pad=2, dil=2, out_dtype=torch.float32)
            y2, col = ops.deformable_conv(y1.permute(0, 3, 1, 2), off.permute(0, 3, 1, 2), t.w(nb), t.conv_bias[nb],
                                          3, 1, 2, 2, 4, relu=True, want_col=True)
            return y2.permute(0, 2, 3, 1), (off, col)      # (the sampled column matrix rides along to the backward: the weight gradient's X operand)

        def unit_fn(x, unit):
            nonlocal y_pre
            nm, mc = unit[1], unit[3]

            def chain(y2, sc):
                ch = t.chain_units.get(nm)
                if ch is None or not ops.chain_worthwhile(y2.numel() // y2.shape[-1], mc):
                    return None
                # expand + shortcut + ReLU and (inside a stage) the NEXT unit's reduce + ReLU in one pixel-wise kernel; every activation
                # the backward needs (x_next, mid1_next) is still written, nothing is overwritten in place
                w1f = t._fragpack.get('w1:' + ch[1]) if ch[0] else None
                b1 = t.conv_bias['res%s_branch2a' % ch[1]] if ch[0] else None
                return ops.bottleneck_chain(y2, sc.contiguous(), t._fragpack.get('w3:' + nm), w1f, t.conv_bias['res%s_branch2c' % nm], b1)
            kept = []
            out, y_pre = bottleneck_unit(t._conv, x, unit, y_pre, deform=deform if t.cfg.dcn else None, expand=chain, kept=kept)
            y1, y2, off = kept
            saved.append(SavedUnit(unit[0], nm, unit[5], unit[6], unit[7], x, y1, y2, out, off))
            return out
        # (fixed res2 ran inside forward_res2; a trainable one takes the same unit path as res3 .. res5, on the per-layer convolutions:
        # its block boundaries have no fragment copies in _fragpack, and the quarter form is not used)
        conv5, conv4, ends = walk_units([u for u in t.units if u[0] > 2 or t.res2_trainable], x, unit_fn, at_conv4)
        ends[5] = conv5
        return conv5, conv4, saved, ends

    def _stem_forward(self, data, im_info, saved):
        """Trainable stem: the three-launch form (pack, 7x7 / 2 convolution WITHOUT bias and ReLU, bias + ReLU + pool1) on the trainer's conv1,
        keeping what its adjoint reads (appended to `saved` as a SavedStem).  -> pooled NHWC map."""
        t = self.t
        fb = t._frozen_backbone
        img = fb._float_image(data, im_info, torch.float32)
        w = t.w('conv1').view(64, 7, 7, 3)                    # folded weights, (ty, tx, c) columns
        bias = t.conv_bias['conv1']
        if t.trunk_fp32:           # exact-fp32 convolution on the image zero-padded to 16 channels, relnet_maxpool_nhwc_f32, bias + ReLU
            B, Cin, H, W = img.shape
            x = torch.zeros((B, H, W, 16), device=img.device, dtype=torch.float32)
            x[..., :Cin] = img.permute(0, 2, 3, 1)
            wz = torch.zeros((64, 7, 7, 16), device=img.device, dtype=torch.float32)
            wz[..., :3] = w
            conv = ops.conv2d_nhwc_f32(x, wz.view(64, -1), None, ksize=7, stride=2, pad=3)
            out = torch.relu_(ops.maxpool_nhwc_f32(conv, 3, 2) + bias)
            saved.append(SavedStem(img, conv, out))
            return out
        w256 = torch.zeros((64, 8, 8, 4), device=img.device, dtype=torch.bfloat16)      # ops.pack_stem_weight's layout, from the working copy
        w256[:, :7, :7, :3] = w
        conv, packed = ops.stem_conv7(img, w256.view(64, 256), None, relu=False, want_packed=True)
        out = ops.stem_bias_relu_pool(conv, bias)
        saved.append(SavedStem(packed, conv, out))
        return out

    def _stem_backward(self, stem, d_out):
        """d_out = gradient of the pooled map -> conv1's weight gradient (conv1 reads the image: no data gradient)."""
        t = self.t
        d_conv = ops.stem_pool_bwd(stem.conv, stem.out, d_out.contiguous())
        g, scale, _ = t._wg('conv1', t.bn_scale['conv1'])
        if not t.trunk_fp32:
            ops.stem_wgrad(stem.image, d_conv, g, scale)
            return
        # float32 trunk (parity tests): conv1's column matrix by unfold, the product on the float32 GEMM
        B = stem.image.shape[0]
        col = F.unfold(stem.image, 7, padding=3, stride=2)                                   # [B, (c, ty, tx), pixels]
        col = col.view(B, 3, 49, -1).permute(0, 3, 2, 1).reshape(-1, 147)                    # [pixels, (ty, tx, c)]
        colp = torch.zeros((col.shape[0], 160), device=col.device, dtype=torch.float32)
        colp[:, :147] = col
        dw = T.wgrad(d_conv.reshape(-1, 64), colp)
        g.add_(dw[:, :147] * (scale * scale).view(-1, 1))

    def backward(self, saved, d_x, inject):
        """res5 -> res3 backward.  d_x = gradient of the last unit's output; inject[unit] = extra gradient of that unit's output."""
        t = self.t
        stem = None
        if isinstance(saved[0], SavedStem):       # trainable conv1: its adjoint follows res2a's
            stem, saved = saved[0], saved[1:]
        B = saved[0].x.shape[0]
        bt = torch.bfloat16
        # trunk: res5 -> res3.  Gradient buckets are announced as they complete (heads first; with DCN the res5 offset
        # convolutions live in the heads bucket, which is then complete only after res5): dist.BucketedAllReduce overlaps
        # each bucket's all-reduce with the rest of the backward pass
        dcn = t.cfg.dcn
        t._grad_buckets()
        if not dcn:
            t._bucket_ready('heads')
        prev_bucket = None
        masked = False            # d_x already carries the ReLU mask of the unit's output (relnet_gemm_nt_mask of the unit after it)
        order = list(reversed(saved))
        for pos, s in enumerate(order):
            nm, x_in, y1, y2 = s.nm, s.x, s.y1, s.y2
            bucket = t._unit_bucket[nm]
            if prev_bucket is not None and bucket != prev_bucket:
                if dcn and prev_bucket == 'res5':
                    t._bucket_ready('res5', 'heads')        # both complete at this point: one cut, two collectives
                else:
                    t._bucket_ready(prev_bucket)
            prev_bucket = bucket
            n1, na, nb, nc_ = 'res%s_branch1' % nm, 'res%s_branch2a' % nm, 'res%s_branch2b' % nm, 'res%s_branch2c' % nm
            if inject.get(nm) is not None:       # a second consumer of this unit's output (RPN head at conv4, FPN laterals)
                assert not masked
                d_x = inject[nm] if d_x is None else d_x + inject[nm]
            g_out = d_x if masked else T.relu_bwd(d_x, s.out)
            masked = False
            # (ReLU masks of the two inner activations ride in the data-gradient kernels' epilogues)
            g_y2, dw = T.conv1x1_bwd(y2, t.w(nc_), g_out, w_t=t.wt(nc_), keep_splits=True, wgrad_to=t._wg(nc_, t.bn_scale[nc_]), relu_mask=y2)
            if s.off is not None:          # deformable branch2b: data + offset gradients, then the offset conv's own backward
                off, col = s.off
                gd, goff, dw = ops.deformable_conv_bwd(y1.permute(0, 3, 1, 2), off.permute(0, 3, 1, 2), t.w(nb),
                                                       g_y2.permute(0, 3, 1, 2), 3, 1, 2, 2, 4, col=col)
                t._add_wgrad(nb, dw, t.bn_scale[nb])
                no = nb + '_offset'
                goff_p = torch.zeros((B, off.shape[1], off.shape[2], 128), device=off.device, dtype=bt)   # 72 -> 128 channels
                goff_p[..., :72] = goff
                wd_ = t.w(no).view(72, 3, 3, -1).flip(1, 2).permute(3, 1, 2, 0)                     # [Cin,3,3,72]
                wdp = torch.zeros((wd_.shape[0], 3, 3, 128), device=off.device, dtype=bt); wdp[..., :72] = wd_
                d_off_in, dwo = T.conv3x3_bwd(y1, wdp.reshape(wd_.shape[0], -1).contiguous(), goff_p, dil=2, keep_splits=True)
                t._add_wgrad(no, dwo.sum(0)[:72]); t._add_bgrad(no, goff.sum((0, 1, 2)))
                d_y1 = (gd + d_off_in.float()).to(bt).contiguous()
                g_y1 = T.relu_bwd(d_y1, y1)
            else:
                g_y1, dw = T.conv3x3_bwd(y1, self._dgrad_w(nb, y2.shape[3]), g_y2, dil=s.dil, keep_splits=True, wgrad_to=t._wg(nb, t.bn_scale[nb]),
                                         relu_mask=y1)
            prev_nm = order[pos + 1].nm if pos + 1 < len(order) else None
            if s.proj:
                # this unit's input has no trainable layer below it -> no data gradient: res3a above a fixed res2 (every shipped list), res2a
                # above a fixed conv1
                first = (s.stage == 3 and not t.res2_trainable) or (s.stage == 2 and not t.stem_trainable)
                # both branches read the same (sampled) input: their data gradients are summed in the second GEMM's epilogue -- at the SAMPLED
                # resolution for a stride-2 unit, then scattered to the input's resolution once, with the previous unit's ReLU mask in the same
                # pass when that output has no other consumer (was: 2 zero fills + 2 strided copies + a full-resolution add + relu_bwd)
                stride = s.stride
                lr = stride != 1
                # a second consumer's gradient of this unit's INPUT (the RPN head at conv4, in front of the stride-1 res5a) rides in the first
                # GEMM's epilogue; the input's ReLU mask can then ride in the second one's
                inj = inject.get(prev_nm) if (stride == 1 and not first and prev_nm is not None) else None
                fold = inj is not None and inj.dtype == g_y1.dtype and tuple(inj.shape) == tuple(x_in.shape) and inj.is_contiguous()
                d_a, dw = T.conv1x1_bwd(x_in, t.w(na), g_y1, stride=stride, need_dx=not first, w_t=t.wt(na), keep_splits=True, wgrad_to=t._wg(na, t.bn_scale[na]),
                                        dx_add=inj if fold else None, low_res=lr)
                if fold:
                    inject = {k: v for k, v in inject.items() if k != prev_nm}
                can_mask = t.mask_epilogue and not first and prev_nm is not None and inject.get(prev_nm) is None
                d_s, dw = T.conv1x1_bwd(x_in, t.w(n1), g_out, stride=stride, need_dx=not first, w_t=t.wt(n1),
                                        dx_add=None if first else d_a, keep_splits=True, wgrad_to=t._wg(n1, t.bn_scale[n1]), low_res=lr,
                                        out_mask=x_in if (can_mask and stride == 1) else None)
                d_x = None if first else d_s
                masked = can_mask and stride == 1
                if lr and not first:
                    d_x = T.strided_scatter(d_s, tuple(x_in.shape), stride, mask=x_in if can_mask else None)
                    masked = can_mask
            else:
                # identity shortcut: d x_in = g_y1 W1 + g_out; x_in is the previous unit's ReLU output, so its mask can ride in this GEMM's
                # epilogue -- unless that output has a second consumer whose gradient must be added before the mask (inject)
                can_mask = t.mask_epilogue and prev_nm is not None and inject.get(prev_nm) is None
                d_x, dw = T.conv1x1_bwd(x_in, t.w(na), g_y1, dx_add=g_out, w_t=t.wt(na), keep_splits=True, wgrad_to=t._wg(na, t.bn_scale[na]),
                                        out_mask=x_in if can_mask else None)
                masked = can_mask
        if stem is not None:          # d_x: gradient of the pooled map (res2a's two branches summed, unmasked: pool_bwd applies out > 0)
            self._stem_backward(stem, d_x)
        t._bucket_ready(prev_bucket)

    # ---- FPN neck --------------------------------------------------------------------------------------------
    def neck_forward(self, ends):
        """ends {2, 3, 4, 5: stage output} -> (feats {4, 8, 16, 32: pyramid map}, the context of `neck_backward`: lateral inputs and tops)."""
        t = self.t
        src = {32: ends[5], 16: ends[4], 8: ends[3], 4: ends[2]}
        if t.trunk_fp32:             # float32 trunk (parity tests): bf16 copies for the bf16 neck / heads
            src = {k: v.to(torch.bfloat16) for k, v in src.items()}
        tops, feats = fpn_neck(t._conv, ops.upsample2x_add_, src[32], {4: src[16], 3: src[8], 2: src[4]})
        return feats, (src, tops)

    def neck_backward(self, ctx, d_feats):
        """d_feats {4, 8, 16, 32: gradient of the pyramid map}: the top-down pathway reversed, finest level first, gradients flowing up to the
        coarser tops.  -> (gradient of conv5, inject = {'4b22', '3b3': gradient of that unit's output} for `backward`; res2c is frozen)."""
        t = self.t
        src, tops = ctx
        bt = torch.bfloat16
        d_tops, inject, d_c5 = {}, {}, None
        for lvl in (4, 8, 16, 32):
            n3, n1 = 'fpn_ft%d_3x3' % lvl, 'fpn_ft%d_1x1' % lvl
            d_top, dw = T.conv3x3_bwd(tops[lvl], self._dgrad_w(n3, 256), d_feats[lvl], dil=1, keep_splits=True, wgrad_to=t._wg(n3))
            T.colsum_add(d_feats[lvl], *t._bg(n3))             # (bias gradients: the bucket's grouped column-sum launch)
            if lvl in d_tops:                                    # + the gradient that came down from the finer level (fp32 block sums)
                d_top = torch.add(d_top, d_tops[lvl]).to(bt)
            if lvl < 32:       # tops[lvl] = lateral + up2x(tops[2 lvl]): adjoint of nearest upsampling = 2x2 block sums (fp32 accumulation, read as bf16)
                Bh, Hh, Wh, Ch = d_top.shape
                d_tops[lvl * 2] = d_top.view(Bh, Hh // 2, 2, Wh // 2, 2, Ch).sum((2, 4), dtype=torch.float32)
            d_top = d_top.contiguous()
            d_src, dw = T.conv1x1_bwd(src[lvl], t.w(n1), d_top, need_dx=(lvl != 4), w_t=t.wt(n1), keep_splits=True, wgrad_to=t._wg(n1))   # res2c is frozen
            T.colsum_add(d_top, *t._bg(n1))
            if lvl == 32:
                d_c5 = d_src
            elif lvl == 16:
                inject['4b22'] = d_src
            elif lvl == 8:
                inject['3b3'] = d_src
        if t.trunk_fp32:
            d_c5, inject = d_c5.float(), {k: v.float() for k, v in inject.items()}
        return d_c5, inject

    # ---- RPN head --------------------------------------------------------------------------------------------
    def rpn_forward(self, conv4):
        """-> (r, rpn [B,h,w,2A | 4A] float32): backbone.rpn_head on the trainer's weights."""
        return rpn_head(self.t._conv, conv4)

    def rpn_backward(self, conv4, r, d_rpn):
        """RPN head backward (joins the trunk at conv4), and with it the two RPN weight gradients as their own grouped launch on
        RPN_WGRAD_WORKGROUPS workgroups.  -> dict(g_r, d_conv4_rpn, rq_keep: what that launch reads, to be kept alive by the caller)."""
        t = self.t
        rq = ops.WgradQueue(deterministic=t.deterministic)
        wg = lambda n: t._wg(n)[:2] + (rq,)
        g_r, dw = T.conv1x1_bwd(r, t.w('rpn_out'), d_rpn, w_t=t.wt('rpn_out'), keep_splits=True, wgrad_to=wg('rpn_out'), relu_mask=r)
        T.colsum_add(d_rpn, *t._bg('rpn_out'))
        d_conv4_rpn, dw = T.conv3x3_bwd(conv4, self._dgrad_w('rpn_conv_3x3', 512), g_r, dil=1, keep_splits=True, wgrad_to=wg('rpn_conv_3x3'))
        T.colsum_add(g_r, *t._bg('rpn_conv_3x3'))
        return dict(g_r=g_r, d_conv4_rpn=d_conv4_rpn, rq_keep=rq.flush(workgroups=RPN_WGRAD_WORKGROUPS))
