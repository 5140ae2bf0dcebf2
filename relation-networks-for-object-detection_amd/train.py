"""End-to-end training step of the relation network (SURVEY.md section 8, rows A10 + A13), one process per GPU.

Graph: the TRAIN branch of relation_rcnn/symbols/resnet_v1_101_rcnn_attention_1024_pairwise_position_multi_head_16.py
:176-322 (reference config experiments/relation_rcnn/cfgs/resnet_v1_101_coco_trainvalminus_rcnn_end2end_relation_
8epoch.yaml): backbone -> RPN losses + proposal -> proposal_target (300 proposals + gt rows, BATCH_ROIS -1) ->
ROIPooling -> fc_new_1 -> relation_1 -> fc_new_2 -> relation_2 (keys = the first 300 rows) -> cls_score / bbox_pred
-> BoxAnnotatorOHEM (128) -> SoftmaxOutput / smooth_l1 losses; then the adjoint of all of it, ONE summed all-reduce
of the trainable gradients (core/module.py + kvstore 'device' in the reference, rescale_grad = 1.0) and
mx.optimizer.SGD (momentum 0.9, wd 5e-4; train_end2end.py:163-168).  Frozen, as cfgs/*.yaml:23-29: conv1, res2 and
every BatchNorm gamma / beta (a cfg.fixed_params list without res2 / conv1 trains them too: check_fixed_params).  With cfg.learn_nms the learn-NMS head's train branch (symbols/..._learn_nms.py:424-551:
per-class sort, rank + appearance embedding, class-batched relation module, sigmoid x score, pos / neg log losses
against nms_multi_target) is trained jointly = BASELINE configs[2].

MI355X-first choices:
  * master weights live in ONE flat fp32 buffer already in the kernels' layouts (convs [Cout][R][S][Cin] with the
    frozen BatchNorm scale folded in, FCs [out][in]); momentum, gradients and the bf16 working copy are flat buffers of
    the same shape, so the optimizer is one launch and the all-reduce one collective over 288 GB-class HBM;
  * folding the frozen BN scale s into w' = w s is exact: dL/dw = s dL/dw', so SGD on w' uses the gradient s^2 dL/dw'
    and the same weight decay; `export_params` divides the scale out again;
  * activations are kept in HBM between forward and backward (~0.45 GB / image, bf16); the relation modules are
    recomputed from their inputs instead of storing [16, N, M] maps.
"""

import numpy as np
import torch

from . import ops, losses, train_ops as T
from . import dist as D
from .backbone import unit_names, conv_bn_names, fold_bn, EPS, TrunkTrain
from .relation import BoxHeadTrain
from .detector import Config, fc1_channels_last_perm
from .learn_nms import LearnNMSTrain, rank_embedding
from .pooling import RoiPooling
from .operator_py.proposal import generate_anchors, propose_batch


class TrainConfig(Config):
    rpn_batch_size = 256          # TRAIN.RPN_BATCH_SIZE
    batch_rois_ohem = 128         # TRAIN.BATCH_ROIS_OHEM
    batch_rois = -1               # -1: every proposal + the gt rows (TRAIN.BATCH_ROIS of the shipped yamls).  R > 0: R sampled rois PER IMAGE
                                  # (TRAIN.BATCH_ROIS // TRAIN.BATCH_IMAGES; core/rcnn.py:329-397 sample_rois), plain heads only
    fg_fraction = 0.25            # TRAIN.FG_FRACTION: at most round(fg_fraction * batch_rois) sampled rois are foreground
    fg_thresh = 0.5               # TRAIN.FG_THRESH
    bg_thresh_lo = 0.0            # TRAIN.BG_THRESH_LO (background = overlap in [bg_thresh_lo, BG_THRESH_HI 0.5))
    lr = 0.0005
    momentum = 0.9
    wd = 0.0005
    nms_loss_scale = 1.0          # TRAIN.nms_loss_scale
    nms_pos_scale = 4.0           # TRAIN.nms_pos_scale
    nms_eps = 1e-8
    bbox_means = (0.0, 0.0, 0.0, 0.0)
    bbox_stds = (0.1, 0.1, 0.2, 0.2)
    relation = True               # two relation modules in the 2FC head (False: the plain head of resnet_v1_101_rcnn_learn_nms_1024_...)
    enable_ohem = True            # TRAIN.ENABLE_OHEM (False: SoftmaxOutput over all rois, bbox loss scaled by 1 / 300)
    fixed_params = None           # network.FIXED_PARAMS of the experiment file (None: dist.FIXED_PARAMS, the end2end yamls' list).  A list without
                                  # 'res2' (and 'conv1') trains them too, e.g. ['gamma', 'beta'], config/config.py:40 (check_fixed_params)
    deterministic = False         # True: every float accumulation of the step whose order the hardware would decide (float atomics: ROI pooling
                                  # backward, bias-gradient column sums, loss scalars, the geometry backward, the learn-NMS take adjoint, the
                                  # stream-K weight-gradient flush) runs its ordered form -- two steps from the same state give the same bits
                                  # (DESIGN.md section 9).  C4 graphs with ROIPooling only: dcn, roi_align and FPNTrainer are refused


def conv4_hw(h, w):
    """Spatial size of conv4 (stride 16) for an h x w image: the stem's pooled map (conv1 7x7 / 2, pool1 3x3 / 2), then the stride-2
    res3a and res4a."""
    half = lambda n: (n - 1) // 2 + 1
    hp, wp = ops._stem_pooled_hw(h, w)
    return half(half(hp)), half(half(wp))


def all_reduce_sum(*buffers):
    """SUM each flat gradient buffer over the ranks (no-op in a single process): the whole data-parallel exchange of a
    training step is these two collectives (weights 271 MB, biases 0.1 MB)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        for b in buffers:
            dist.all_reduce(b, op=dist.ReduceOp.SUM)
        if buffers and buffers[0].is_cuda and dist.get_backend() != 'nccl':
            torch.cuda.synchronize()            # gloo on device tensors (one-GPU test path), see dist.BucketedAllReduce.finish


def box_target_layout(cfg):
    """The regression-target layout the trainers ask ops.proposal_target for (lib/bbox/bbox_regression.py:129-140): [R, 8] with the target
    at columns 4..7 when class agnostic, else [R, 4 * num_classes] with the four entries at 4 * label."""
    agnostic = bool(getattr(cfg, 'class_agnostic', True))
    return dict(num_reg=2 if agnostic else cfg.num_classes, class_agnostic=agnostic)


def check_box_head(cfg, params):
    """cfg.class_agnostic, cfg.num_classes and the parameters' cls_score / bbox_pred rows must describe one head (symbols/...:157
    num_reg_classes = 2 if CLASS_AGNOSTIC else num_classes)."""
    rows, nc = int(params['bbox_pred_weight'].shape[0]), int(params['cls_score_weight'].shape[0])
    agnostic = bool(getattr(cfg, 'class_agnostic', True))
    want = 8 if agnostic else 4 * nc
    if rows != want or (not agnostic and nc != cfg.num_classes):
        raise ValueError("class_agnostic=%s with %d classes (cfg.num_classes %d) needs a bbox_pred_weight of %d rows, got %d"
                         % (agnostic, nc, cfg.num_classes, want, rows))


def check_deterministic(cfg):
    """cfg.deterministic covers the C4 graphs with ROIPooling, class-agnostic or class-specific (cfg.class_agnostic = False adds no float
    accumulation: wider targets, the per-class geometry branch of the learn-NMS head).  The other pooling operators and the deformable convolutions still accumulate
    with float atomics, whose order the hardware decides: refused by name rather than silently not reproducible."""
    if not getattr(cfg, 'deterministic', False):
        return
    if getattr(cfg, 'fpn', False):
        raise ValueError("deterministic training does not cover the FPN graphs: roi_pool_fpn_bwd (and roi_align_bwd with cfg.roi_align) accumulate with float atomics")
    if getattr(cfg, 'dcn', False):
        raise ValueError("deterministic training does not cover cfg.dcn: deformable_psroi_pool_bwd and deformable_col2im accumulate with float atomics")
    if getattr(cfg, 'roi_align', False):
        raise ValueError("deterministic training does not cover cfg.roi_align: roi_align_bwd accumulates with float atomics")


def check_fixed_params(cfg):
    """cfg.fixed_params (network.FIXED_PARAMS; a parameter is fixed when ANY pattern is a substring of its name, core/module.py:753-764) as
    far as it concerns the bottom of the trunk.  -> (conv1 is trainable, res2 is trainable).  Built: the shipped lists (both fixed), res2
    trainable above a fixed conv1, both trainable.  Refused by name: a trainable conv1 under a fixed res2, a list that leaves BatchNorm
    gamma / beta trainable (the affine terms and the statistics stay fixed, folded into the convolutions), and a trainable res2 in the FPN
    graphs."""
    fixed = getattr(cfg, 'fixed_params', None)
    if fixed is None:
        return False, False
    fixed = tuple(fixed)
    for term in ('gamma', 'beta'):
        loose = [n for n in ('bn_conv1_' + term, 'bn2a_branch1_' + term, 'bn4b7_branch2b_' + term, 'bn5c_branch2c_' + term) if D.is_trainable(n, fixed)]
        if loose:
            raise ValueError("fixed_params %s leaves BatchNorm %s trainable (%s): the BatchNorm affine terms and statistics are folded into the "
                             "convolutions and stay fixed -- 'gamma' and 'beta' are missing from the list" % (list(fixed), term, loose[0]))
    conv1 = D.is_trainable('conv1_weight', fixed)
    res2 = [D.is_trainable(conv + '_weight', fixed) for conv, _, _, _, _ in conv_bn_names() if conv.startswith('res2')]
    if any(res2) and not all(res2):
        raise ValueError("fixed_params %s fixes some res2 convolutions and not others: res2 is trainable or fixed as a whole -- the pattern 'res2' "
                         "is missing" % (list(fixed),))
    res2 = all(res2)
    if conv1 and not res2:
        raise ValueError("fixed_params %s leaves conv1 trainable under a fixed res2: conv1's gradient needs the data gradient through res2, which a "
                         "fixed res2 (run on the inference kernels) does not produce -- 'conv1' is missing from the list, or 'res2' must leave it" % (list(fixed),))
    if res2 and getattr(cfg, 'fpn', False):
        raise ValueError("fixed_params %s leaves res2 trainable in an FPN graph: the lateral gradient of fpn_ft4_1x1 into res2c is missing "
                         "(FPNTrainer treats res2c as fixed) -- 'res2' and 'conv1' must stay in the list" % (list(fixed),))
    return conv1, res2


def check_batch_rois(cfg):
    """cfg.batch_rois is -1 (every proposal + the gt rows) or the number of sampled rois per image.  The relation modules and the learn-NMS
    head take the first RPN_POST_NMS_TOP_N rows of an image as attention keys / ranked proposals (nongt_dim, symbols/...:220-262): a sampled
    minibatch has no such rows, so those graphs are refused by name (the reference's relation yamls all set BATCH_ROIS -1 for this reason)."""
    r = int(getattr(cfg, 'batch_rois', -1))
    if r == -1:
        return
    if r <= 0:
        raise ValueError("cfg.batch_rois is -1 or the sampled rois per image (TRAIN.BATCH_ROIS // TRAIN.BATCH_IMAGES > 0), got %d; the -2 and "
                         "< -10 forms of BATCH_ROIS exist on the proposal_target operator only" % r)
    for flag in ('relation', 'learn_nms'):
        if getattr(cfg, flag, flag == 'relation'):
            raise ValueError("cfg.%s with batch_rois = %d: the attention keys are the first RPN_POST_NMS_TOP_N rows of every image, which a "
                             "sampled minibatch does not keep -- these graphs need BATCH_ROIS = -1" % (flag, r))


class _Flat(object):
    """Named fp32 tensors carved out of one flat buffer (64-element aligned slices)."""

    def __init__(self, named, device):
        self.slices, off = {}, 0
        for n, t in named:
            self.slices[n] = (off, tuple(t.shape))
            off += (t.numel() + 63) // 64 * 64
        self.size = off
        self.master = torch.zeros(off, device=device, dtype=torch.float32)
        for n, t in named:
            self.view(self.master, n).copy_(t)
        self.mom = torch.zeros_like(self.master)
        self.grad = torch.zeros_like(self.master)
        self.work = self.master.to(torch.bfloat16)

    def view(self, buf, name):
        off, shape = self.slices[name]
        n = 1
        for d in shape:
            n *= d
        return buf[off:off + n].view(shape)


class GradGuard(object):
    """Device-side guard of `Trainer.update()` (csrc/guard.hip): the global L2 norm and the non-finite count of all trainable
    gradients are measured after the all-reduce (every rank decides from the same numbers), the WHOLE update is skipped when any
    element is inf / NaN -- master weights, momentum and bf16 copies stay bit-unchanged -- and the gradient can be clipped:

      max_norm       by global norm, torch.nn.utils.clip_grad_norm_'s rule: every gradient times min(1, max_norm / (norm + 1e-6))
      clip_gradient  element-wise, mx.optimizer.SGD's: mom = momentum mom - lr (clip(rescale_grad grad, +-c) + wd w)
                     (with both, the global scale is applied first)

    None of it synchronises with the host or allocates per step (the workspace is sized when the guard first meets a trainer's
    ranges).  `GradGuard()` only measures and skips: a finite gradient then gives the bits of the unguarded update.  The host never
    learns that a step was skipped: `Trainer.step_count` advances all the same, so a learning-rate schedule stays a function of the
    number of calls.  `report()` is the one place that synchronises."""

    def __init__(self, max_norm=None, clip_gradient=None):
        assert max_norm is None or max_norm > 0, "max_norm must be positive (None: no global-norm clipping)"
        assert clip_gradient is None or clip_gradient >= 0, "clip_gradient must not be negative (None: no element-wise clipping)"
        self.max_norm, self.clip_gradient = max_norm, clip_gradient
        self.state = self.workspace = None
        self._cursor = 0

    def bind(self, device):
        """Create the guard state on `device` (done by the trainer on first use)."""
        if self.state is None or self.state.device != torch.device(device):
            self.state = T.grad_guard_state(device)
            self.workspace = None
        return self

    def begin(self, slots):
        """Start the statistics of one step that will write `slots` slots in all."""
        if self.workspace is None or self.workspace.numel() * 8 < slots * T.GUARD_SLOT_BYTES:
            self.workspace = T.grad_guard_workspace(slots, self.state.device)
        self._cursor = 0

    def stats(self, views):
        for i in range(0, len(views), T.GUARD_MAX_RANGES):
            self._cursor += T.grad_stats(views[i:i + T.GUARD_MAX_RANGES], self.workspace, self._cursor)

    def decide(self):
        T.grad_guard_decide(self.workspace, self._cursor, self.state, self.max_norm or 0.0)

    def reset(self):
        """Zero the totals (and the last step's figures)."""
        if self.state is not None:
            self.state.copy_(T.grad_guard_state(self.state.device))

    def report(self):
        """Totals since the last reset, read back from the device (synchronises).  mean_norm / max_norm_seen are over the steps that
        were not skipped; last_norm is the norm of the finite elements when the last step was skipped."""
        if self.state is None:
            return {'steps': 0, 'skipped': 0, 'clipped': 0, 'last_norm': 0.0, 'last_nonfinite': 0, 'mean_norm': 0.0, 'max_norm_seen': 0.0}
        s = self.state.cpu()
        f = s.view(torch.float64)
        steps, skipped, clipped = int(s[3]), int(s[4]), int(s[5])
        return {'steps': steps, 'skipped': skipped, 'clipped': clipped, 'last_norm': float(f[1]), 'last_nonfinite': int(s[2]),
                'mean_norm': float(f[6]) / max(steps - skipped, 1), 'max_norm_seen': float(f[7])}


class Trainer(object):
    def __init__(self, params, cfg=None, device='cuda', im_hw=(600, 1000), metrics=None, guard=None):
        """guard: a GradGuard (default None: the optimizer applies whatever the gradient buffers hold); `tr.guard` may also be set or
        cleared between updates.
        metrics: a metric.TrainMetrics (default None: no metric launch, no extra output).  With one, every step adds the reference's
        training metrics into its device accumulator -- no host synchronisation, also inside a CapturedStep -- and `out` additionally carries
        rpn_cls_prob, rpn_label, cls_prob, nms_conditional_score and the loss tensors behind the loss scalars (rpn_bbox_loss_map, bbox_loss_map,
        nms_pos_loss_map, nms_neg_loss_map): the output list of the reference's train graph, which metric.py's host classes take."""
        self.cfg = cfg or TrainConfig()
        check_deterministic(self.cfg)       # (its user-facing messages come before the pooler's assertions)
        c = self.cfg
        # conv1 / res2 join the trainable trunk when network.FIXED_PARAMS leaves them out (both False for every shipped list)
        self.stem_trainable, self.res2_trainable = check_fixed_params(c)
        self.deterministic = bool(getattr(c, 'deterministic', False))       # read ONCE: every site below routes on this attribute
        self.fpn = bool(getattr(c, 'fpn', False))
        self.pool = RoiPooling(c, self.scales if self.fpn else (1.0 / c.feat_stride,), deterministic=self.deterministic)
        check_batch_rois(self.cfg)
        check_box_head(self.cfg, params)
        self.device, self.im_hw = device, im_hw
        self.class_agnostic = bool(getattr(c, 'class_agnostic', True))
        dev = device
        f32 = lambda t: torch.as_tensor(t).to(dev, torch.float32).contiguous()
        self.relation = bool(getattr(c, 'relation', True))
        # cfg.trunk_fp32 (parity tests only): conv1 .. res5 forward AND backward in float32 on the exact-fp32 MFMA kernels
        # (relnet_conv2d_nhwc_f32 / relnet_gemm_nt f32, master weights read directly, no chain kernels, no fused ReLU-mask epilogue) with
        # the SAME wiring code (_trunk_forward / _trunk_backward / train_ops) -- removes the bf16 noise of ~100 layers from the
        # end-to-end gradient comparison, so that the trunk's wiring is pinned to float64 autograd at 1e-4 instead of 2e-2
        self.trunk_fp32 = bool(getattr(c, 'trunk_fp32', False))
        assert not (self.trunk_fp32 and getattr(c, 'dcn', False)), "trunk_fp32 covers the plain and FPN trunks"
        if torch.device(dev).type == 'cuda':
            ops.asm_selfcheck()
        self.units = unit_names(self.fpn)
        # the tensors this step never changes (frozen by name, cfgs/*.yaml:23-29, and the BatchNorm running statistics):
        # kept on the host under the reference's names so that a checkpoint holds the complete arg / aux dictionaries
        # (a list that leaves res2 / conv1 trainable is followed here too: their initial tensors are not kept, the checkpoint holds the updated ones)
        src_fixed = tuple(c.fixed_params) if self.res2_trainable else D.FIXED_PARAMS
        self._fixed_src = {k: torch.as_tensor(v).detach().to('cpu', torch.float32).clone() for k, v in params.items()
                           if ('moving_' in k) or not D.is_trainable(k, src_fixed)}
        # ---- frozen part: conv1 + res2 never change under the shipped lists; they run on the inference kernels (fused stem, halo 3x3, chain
        # kernels) of a Backbone built from the same parameters with folded BN.  (With a trainable res2 it still runs a fixed conv1's fused
        # stem and the uint8 image transform.)
        from .backbone import Backbone
        self._frozen_backbone = Backbone(params, dtype=torch.float32 if self.trunk_fp32 else torch.bfloat16, device=dev, fpn=self.fpn,
                                         frozen_only=True, pixel_means=c.pixel_means)
        weights, biases = [], []
        self.bn_scale, self.conv_bias, self.ksize = {}, {}, {'rpn_conv_3x3': 3, 'rpn_out': 1, 'conv_new_1': 1}
        for conv, bn, oc, ic, k in conv_bn_names():
            if (conv == 'conv1' and not self.stem_trainable) or (conv.startswith('res2') and not self.res2_trainable):
                continue
            w, b = fold_bn(params[conv + '_weight'], params[bn + '_gamma'], params[bn + '_beta'],
                           params[bn + '_moving_mean'], params[bn + '_moving_var'])
            self.ksize[conv] = k
            self.conv_bias[conv] = f32(b)                                   # beta - mean * s: frozen
            s = (params[bn + '_gamma'].double() / torch.sqrt(params[bn + '_moving_var'].double() + EPS)).float()
            self.bn_scale[conv] = f32(s)
            weights.append((conv, w.permute(0, 2, 3, 1).reshape(oc, -1)))
        # ---- RPN head, conv_new_1, 2FC head, relation modules
        def conv_w(name):
            w = params[name + '_weight']
            return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
        if self.fpn:        # FPN neck (symbols/..._fpn_...:804-840); no RPN in these graphs (HAS_RPN: false)
            for lvl in (32, 16, 8, 4):
                for k_, ks in (('1x1', 1), ('3x3', 3)):
                    n = 'fpn_ft%d_%s' % (lvl, k_)
                    weights.append((n, conv_w(n))); biases.append((n, params[n + '_bias'])); self.ksize[n] = ks
            fc1n, fc2n = 'roi_pool_fc1', 'roi_pool_fc2'
        else:
            weights.append(('rpn_conv_3x3', conv_w('rpn_conv_3x3'))); biases.append(('rpn_conv_3x3', params['rpn_conv_3x3_bias']))
            self.na2 = params['rpn_cls_score_weight'].shape[0]
            weights.append(('rpn_out', torch.cat([conv_w('rpn_cls_score'), conv_w('rpn_bbox_pred')], 0)))
            biases.append(('rpn_out', torch.cat([params['rpn_cls_score_bias'], params['rpn_bbox_pred_bias']], 0)))
            weights.append(('conv_new_1', conv_w('conv_new_1'))); biases.append(('conv_new_1', params['conv_new_1_bias']))
            fc1n, fc2n = 'fc_new_1', 'fc_new_2'
        self.fc_names = (fc1n, fc2n)
        self.fc1_perm = fc1_channels_last_perm()
        weights.append(('fc_new_1', params[fc1n + '_weight'][:, self.fc1_perm])); biases.append(('fc_new_1', params[fc1n + '_bias']))
        weights.append(('fc_new_2', params[fc2n + '_weight'])); biases.append(('fc_new_2', params[fc2n + '_bias']))
        self.num_classes = params['cls_score_weight'].shape[0]
        weights.append(('cls_bbox', torch.cat([params['cls_score_weight'], params['bbox_pred_weight']], 0)))
        biases.append(('cls_bbox', torch.cat([params['cls_score_bias'], params['bbox_pred_bias']], 0)))
        for i in ((1, 2) if self.relation else ()):
            weights.append(('qk_%d' % i, torch.cat([params['query_%d_weight' % i], params['key_%d_weight' % i]], 0)))
            biases.append(('qk_%d' % i, torch.cat([params['query_%d_bias' % i], params['key_%d_bias' % i]], 0)))
            wo = params['linear_out_%d_weight' % i]
            weights.append(('linear_out_%d' % i, wo.reshape(wo.shape[0], wo.shape[1])))
            biases.append(('linear_out_%d' % i, params['linear_out_%d_bias' % i]))
            weights.append(('pair_pos_fc1_%d' % i, params['pair_pos_fc1_%d_weight' % i]))
            biases.append(('pair_pos_fc1_%d' % i, params['pair_pos_fc1_%d_bias' % i]))
        if c.dcn:           # deformable res5 (offset convs) + deformable PSROI pooling's offset FC (SYM_DCN_RELNMS:700-746,1073-1080)
            for u in 'abc':
                n = 'res5%s_branch2b_offset' % u
                weights.append((n, conv_w(n))); biases.append((n, params[n + '_bias']))
                self.ksize[n] = 3
        if c.learn_nms:     # learn-NMS head (symbols/..._learn_nms.py:424-551), trained end to end with the detector
            for n in ('nms_rank', 'roi_feat_embedding', 'nms_pair_pos_fc1_1', 'nms_logit'):
                weights.append((n, params[n + '_weight'])); biases.append((n, params[n + '_bias']))
            weights.append(('nms_qk_1', torch.cat([params['nms_query_1_weight'], params['nms_key_1_weight']], 0)))
            biases.append(('nms_qk_1', torch.cat([params['nms_query_1_bias'], params['nms_key_1_bias']], 0)))
            weights.append(('nms_linear_out_1', params['nms_linear_out_1_weight'].reshape(128, 128)))
            biases.append(('nms_linear_out_1', params['nms_linear_out_1_bias']))
            self.rank_emb = rank_embedding(c.first_n, 1024).to(dev, torch.bfloat16).contiguous()
            self._lnms = LearnNMSTrain(self)
        self.lr_mult_tail = None
        if c.dcn:           # `offset` FC has lr_mult = 0.01 (SYM_DCN_RELNMS:1075): keep it LAST so it is one tail range
            weights.append(('offset', params['offset_weight'][:, self.fc1_perm])); biases.append(('offset', params['offset_bias']))
        self.W = _Flat(weights, dev)          # weight decay applies
        self.Bv = _Flat(biases, dev)          # biases: wd_mult 0 (MXNet's rule for names not ending in _weight / _gamma)
        if c.dcn:
            self.lr_mult_tail = (self.W.slices['offset'][0], self.Bv.slices['offset'][0], 0.01)
        # network.FIXED_PARAMS (core/module.py:753-764: a parameter is fixed when ANY pattern is a substring of its name -- 'cls_score' also fixes
        # rpn_cls_score).  The end2end experiments fix conv1 / res2 / the BatchNorm affine terms, which this class never registers as trainable; the
        # learn-NMS-only experiment (..._rcnn_end2end_learn_nms_3epoch.yaml:23-40, JOINT_TRAINING false) fixes the whole detector: what is left are
        # the learn-NMS head's parameters.  A fused slice (rpn_out = rpn_cls_score | rpn_bbox_pred, ...) is frozen when all its members are.
        fixed = tuple(getattr(c, 'fixed_params', None) or D.FIXED_PARAMS)
        members = {'rpn_out': ('rpn_cls_score', 'rpn_bbox_pred'), 'cls_bbox': ('cls_score', 'bbox_pred'), 'fc_new_1': (fc1n,), 'fc_new_2': (fc2n,),
                   'qk_1': ('query_1', 'key_1'), 'qk_2': ('query_2', 'key_2'), 'nms_qk_1': ('nms_query_1', 'nms_key_1')}
        def _frozen(flat_name):
            fr = [not D.is_trainable(m + '_weight', fixed) for m in members.get(flat_name, (flat_name,))]
            assert all(fr) or not any(fr), "FIXED_PARAMS splits the fused slice %s" % flat_name
            return all(fr)
        self.frozen_names = {n for n in self.W.slices if _frozen(n)}
        lnms_names = {'nms_rank', 'roi_feat_embedding', 'nms_pair_pos_fc1_1', 'nms_logit', 'nms_qk_1', 'nms_linear_out_1'}
        # the pruned step: every parameter outside the learn-NMS head is fixed -> no gradient leaves that head, nothing behind it is differentiated
        self.lnms_only = bool(c.learn_nms) and bool(self.frozen_names) and all((n in self.frozen_names) != (n in lnms_names) for n in self.W.slices)
        assert not self.frozen_names or self.lnms_only, "fixed parameter sets other than the end2end yamls' / the learn-NMS-only yaml's are not built: %s" % sorted(self.frozen_names)
        self.anchors_host = generate_anchors(c.feat_stride, c.anchor_ratios, c.anchor_scales)      # float64 [A,4], host (kernel argument)
        self.anchors = torch.as_tensor(self.anchors_host, dtype=torch.float64, device=dev)
        self.step_count = 0
        self.guard = guard
        self.metrics = metrics
        if metrics is not None:         # which metrics exist follows the graph: RPN ones with an RPN in it, NMS ones with the learn-NMS head
            metrics.has_rpn, metrics.has_nms = not self.fpn, bool(c.learn_nms)
        # state that used to be created on first use -- inside a hipGraph capture that turned into a captured fill / mid-capture
        # stream and attribute calls: the device step counter of the anchor sampler, the RPN side stream, the queues of
        # the deferred gradient work -- weight-gradient products and bias-gradient column sums, each launched grouped when a gradient
        # bucket completes (`_flush_wgrads`)
        self._anchor_step = torch.zeros(1, device=dev, dtype=torch.int64)
        self._side = torch.cuda.Stream(device=dev)
        self._wq = ops.WgradQueue(deterministic=self.deterministic)
        self._cq = T.ColsumQueue(deterministic=self.deterministic)
        # every data-parallel rank samples its own fg / bg anchor subsets (cfg.rank_in_anchor_seed = False: the same subsets on every
        # rank, what the two-rank gradient-sum check needs)
        self._rank, self._world = (0, 1) if not getattr(c, 'rank_in_anchor_seed', True) else ((torch.distributed.get_rank(), torch.distributed.get_world_size())
                                   if torch.distributed.is_available() and torch.distributed.is_initialized() else (0, 1))
        # data-gradient copies of the weights (W^T, tap-flipped 3x3 filters): ONE grouped launch per step instead of a
        # transpose / flip / copy per layer inside the backward pass
        self._relayout = ops.WeightRelayout(dev)
        for name in self.W.slices:
            taps = 9 if self.ksize.get(name, 1) == 3 else 1
            group = None
            if name == 'nms_qk_1':                           # learn-NMS module: [Wq; Wk]^T | padded Wout^T (8 real of 64 columns per head)
                self._relayout.add(name, self.w(name), taps=1, pad_co=64, group=('rel_cat_nms', 0, 3 * 1024))
                wo = self.w('nms_linear_out_1')
                for h in range(16):
                    self._relayout.add('nms_lo_h%d' % h, wo[8 * h:8 * h + 8], taps=1, pad_co=8, group=('rel_cat_nms', 2048 + 64 * h, 3 * 1024))
                continue
            if name == 'nms_logit':                          # [T,128] -> [128, 64] (T real columns): data-gradient operand of the learn-NMS logit layer
                self._relayout.add(name, self.w(name), taps=1, pad_co=64)
                continue
            if name.startswith(('pair_pos_fc1', 'nms_')) or name.endswith('_offset') or self._trunk32(name) or name == 'conv1':
                continue                                    # consumed in other layouts (relation_bwd kernels, padded DCN offset convs; float32 trunk);
                                                            # conv1 reads the image: no data gradient
            if name.startswith(('qk_', 'linear_out_')):     # [Wq; Wk]^T | Wout^T side by side: the [1024, 3072] operand of the ONE
                i = name.rsplit('_', 1)[1]                  # projection-backward GEMM of relation module i (relation.GradSink)
                group = ('rel_cat_' + i, 0 if name.startswith('qk_') else self.W.slices['qk_' + i][1][0])
            self._relayout.add(name, self.w(name), taps=taps, pad_co=1 if taps == 9 else 64, group=group)
        self._relayout.build()
        # ---- res3 .. res5, FPN neck, RPN head convolutions and their adjoints (registers the chain kernels' weight copies: _fragpack, chain_units)
        self._trunk = TrunkTrain(self)
        # data gradient through `relu(expand + shortcut)` with the ReLU mask in the GEMM epilogue (relnet_gemm_nt_mask) instead of a
        # separate relnet_relu_bwd pass over three [pixels, 4 mid] maps per unit (off for the float32 trunk)
        self.mask_epilogue = not self.trunk_fp32
        self._scratch_bufs = {}
        self._box_head = BoxHeadTrain(self)

    # ---- accessors ----------------------------------------------------------------------------------------
    def _trunk32(self, name):
        return self.trunk_fp32 and (name.startswith('res') or name == 'conv1') and not name.endswith('_offset')

    def w(self, name):          # bf16 working copy (the float32 master weights for the trunk layers of a cfg.trunk_fp32 trainer)
        return self.W.view(self.W.master if self._trunk32(name) else self.W.work, name)

    def b(self, name):          # fp32 bias
        return self.Bv.view(self.Bv.master, name)

    def wt(self, name):         # data-gradient layout of w(name), refreshed by _relayout.run() at the start of every step
        if self._trunk32(name):
            return None         # (float32 trunk: train_ops transposes / flips the master weights on the fly)
        return self._relayout.get(name)

    def num_trainable(self):
        return sum(int(np.prod(s)) for _, s in self.W.slices.values()) + sum(int(np.prod(s)) for _, s in self.Bv.slices.values())

    def _add_wgrad(self, name, dw, scale_rows=None):
        """dw: the gradient [rows, cols], or the split-K partial sums [splits, rows, cols] of train_ops.wgrad(keep_splits=True)
        (summed, scaled by the folded-BN factor and accumulated by ONE kernel)."""
        if dw is None:              # already accumulated by relnet_wgrad (wgrad_to)
            return
        g = self.W.view(self.W.grad, name)
        if dw.dim() == 3 and dw.is_contiguous() and dw.shape[1] * dw.shape[2] == g.numel() and g.shape[-1] % 4 == 0:
            T.wgrad_accumulate(dw, g, scale_rows)
            return
        if dw.dim() == 3:
            dw = dw.sum(0)
        dw = dw.reshape(g.shape)
        if scale_rows is not None:
            dw = dw * (scale_rows * scale_rows).view(-1, 1)
        g.add_(dw)

    def _wg(self, name, scale_rows=None):
        """(2-D fp32 view of `name`'s slice of the flat gradient buffer, folded-BatchNorm row factor | None): the target
        relnet_wgrad accumulates into (train_ops `wgrad_to` protocol)."""
        g = self.W.view(self.W.grad, name)
        return g.view(g.shape[0], -1), scale_rows, self._wq       # the products wait there for ONE grouped stream-K launch per gradient bucket

    def _flush_wgrads(self):
        """Launch the deferred gradient work of the step so far, on the current stream: the queued bias-gradient column sums
        (relnet_colsum_add_grouped) and weight-gradient products (csrc/wgrad.hip), one grouped launch each.  A gradient bucket is
        complete only after this."""
        self._cq.flush()
        self._wq.flush()

    def _scratch(self, name, shape, dtype):
        """Persistent zero-initialised work buffer (created on first use, i.e. in the eager warm-up step, never inside a capture)."""
        key = (name, tuple(shape), dtype)
        if key not in self._scratch_bufs:
            self._scratch_bufs[key] = torch.zeros(shape, device=self.device, dtype=dtype)
        return self._scratch_bufs[key]

    def _add_bgrad(self, name, db):
        if db is not None:          # (None: already accumulated by T.colsum_add through _bg(name))
            self.Bv.view(self.Bv.grad, name).add_(db.reshape(-1))

    def _bg(self, name):
        """(fp32 view of `name`'s slice of the flat bias-gradient buffer, the step's ColsumQueue): the bias target T.colsum_add(x, *target) /
        linear_bwd(bgrad_to=) / relation.GradSink accumulate into, with the column sums waiting for the bucket's grouped launch."""
        return self.Bv.view(self.Bv.grad, name).view(-1), self._cq

    # ---- forward -------------------------------------------------------------------------------------------
    def _conv(self, x, name, stride=1, pad=0, dil=1, relu=False, resid=None, out_dtype=None):
        """Layer `name` on the working weights; its bias is the folded BatchNorm's frozen one (res3 .. res5) or the layer's own trainable one."""
        bias = self.conv_bias[name] if name in self.conv_bias else self.b(name)
        return ops.conv2d_nhwc(x, self.w(name), bias, ksize=self.ksize.get(name, 1), stride=stride, pad=pad, dil=dil, relu=relu,
                               resid=resid, out_dtype=out_dtype)

    def _trunk_forward(self, data, at_conv4=None, im_info=None):
        return self._trunk.forward(data, at_conv4, im_info)

    def _trunk_backward(self, saved, d_x, inject):
        return self._trunk.backward(saved, d_x, inject)

    def rpn_targets(self, gt_boxes, num_gt, im_info, feat_hw):
        """lib/rpn/rpn.py:80-244 (`assign_anchor`, host numpy inside the reference's AnchorLoader) on the device for the whole
        batch: one C-ABI call, no host round trip.  The random fg / bg subset is keyed by cfg.seed + a device step counter that
        is advanced here, i.e. also by every replay of a captured step."""
        c = self.cfg
        out = ops.assign_anchor(gt_boxes, num_gt, im_info, self.anchors_host, feat_hw, c.feat_stride, c.rpn_batch_size,
                                getattr(c, 'rpn_fg_fraction', 0.5), getattr(c, 'rpn_negative_overlap', 0.3),
                                getattr(c, 'rpn_positive_overlap', 0.7), seed=getattr(c, 'seed', 0) * self._world + self._rank, seed_dev=self._anchor_step)
        self._anchor_step += 1
        return out

    def roi_targets(self, rois, gt_boxes, num_gt, num_rois=None, advance=False):
        """operator_py/proposal_target.py:44-93 on the device: labels and regression targets of the step's rois.  cfg.batch_rois -1: every
        proposal + the gt rows (today's launch).  cfg.batch_rois = R > 0: the sampled minibatch (core/rcnn.py:329-397), keyed like the anchor
        sampler by the trainer's seed + the device step counter AS IT STANDS when this launch runs (after `rpn_targets` of the same step, which
        advances it); advance=True advances it here, for a step in which `rpn_targets` does not run -- so every step, and every replay of a
        captured one, draws a new sample.  Returns (rois_t, label, bbox_target, bbox_weight, keep_index or None)."""
        c = self.cfg
        R = int(getattr(c, 'batch_rois', -1))
        if R <= 0:
            return ops.proposal_target(rois, gt_boxes, num_gt, num_rois=num_rois, **box_target_layout(c)) + (None,)
        o = ops.proposal_target(rois, gt_boxes, num_gt, num_rois=num_rois, batch_rois=R, fg_fraction=c.fg_fraction, fg_thresh=c.fg_thresh,
                                bg_thresh_lo=c.bg_thresh_lo, seed=getattr(c, 'seed', 0) * self._world + self._rank,
                                seed_dev=self._anchor_step, want_index=True, **box_target_layout(c))
        if advance:
            self._anchor_step += 1
        return o

    def forward_backward(self, *args, **kwargs):
        """One forward + backward pass (arguments: see `_forward_backward_impl` of the trainer class).  While it runs, bias-gradient column sums
        and weight-gradient products are queued on the trainer and launched grouped when a gradient bucket completes (`_flush_wgrads`)."""
        try:
            return self._forward_backward_impl(*args, **kwargs)
        finally:
            self._flush_wgrads()        # (nothing is left unless a caller skipped the bucket announcements)

    def _forward_backward_impl(self, data, im_info, gt_boxes, rpn_label=None, rpn_bbox_target=None, rpn_bbox_weight=None, num_gt=None):
        """data [B,3,H,W] fp32 or [B,H,W,3] uint8 BGR HWC (Backbone.forward); gt_boxes [B,G,5]; rpn_label [B, A*h*w] ((a,y,x) order), rpn_bbox_target / weight
        [B, 4A, h, w] (lib/rpn/rpn.py:assign_anchor layouts) -- or None: computed on the device from gt_boxes
        (`rpn_targets`).  Accumulates gradients into the flat buffers and returns the loss values (reference metric names).
        With cfg.batch_rois > 0 the head runs on the sampled rows only (`roi_targets`) and `out` also carries `proposals` [B,N,5] (the RPN's
        output the sample was drawn from) and `keep_index` [B,R] (the candidate -- proposal, or N + gt row -- behind every row)."""
        c = self.cfg
        B = data.shape[0]
        self._grad_buckets().reset()
        self.W.grad.zero_(); self.Bv.grad.zero_()
        self._fragpack.run()            # the fragment-order copies the chain kernels of the forward read
        # The RPN branch (head convolutions, anchor targets, losses, proposals, proposal targets: everything that hangs off conv4)
        # runs on a side stream BESIDE res5 / conv_new_1 -- its top-k / sort / NMS / target kernels are one workgroup per image and
        # leave the GPU idle on their own; fork when conv4 exists, join before ROI pooling (graph edges under capture).
        out = {}
        br = {}
        main, side = torch.cuda.current_stream(), self._side
        nchw = lambda t: t.permute(0, 3, 1, 2)
        # the RPN head's backward runs on the side stream too (not in a learn-NMS-only step: nothing behind that head is differentiated)
        rpn_bwd_side = not self.lnms_only

        early = None
        if rpn_label is None:
            # the anchor targets depend on the ground truth only (lib/rpn/rpn.py:assign_anchor runs in the LOADER in the reference): on the side stream
            # from the very start of the step, beside the stem -- their 0.23 ms (8 images) used to sit between the RPN head and the proposals, on
            # the longer of the two branches that meet at ROI pooling
            side.wait_stream(main)
            with torch.cuda.stream(side):
                early = self.rpn_targets(gt_boxes, num_gt, im_info, conv4_hw(*ops.image_hw(data)))

        def rpn_branch(conv4):
            r, rpn = self._trunk.rpn_forward(conv4)                                                      # [B,h,w,72]
            h, wd_ = rpn.shape[1], rpn.shape[2]
            na2 = self.na2
            lbl, tgt_in, wgt_in = (rpn_label, rpn_bbox_target, rpn_bbox_weight) if early is None else early
            if early is not None and tuple(tgt_in.shape[2:]) != (h, wd_):
                # (never recomputed here: that would advance the anchor sampler's device step counter a second time in this step)
                raise RuntimeError("early RPN anchor targets are %dx%d, conv4 is %dx%d" % (tgt_in.shape[2], tgt_in.shape[3], h, wd_))
            # -- RPN losses (per image, like one image per device in the reference)
            score_nchw = rpn[..., :na2].permute(0, 3, 1, 2).contiguous()                                 # [B,2A,h,w]
            # per-image 'valid' normalisation (one image per executor in the reference) in ONE launch: group = one image's anchors
            rpn_prob, d_score = losses.softmax_output(score_nchw.view(B, 2, -1), lbl, multi_output=True, use_ignore=True,
                                                      ignore_label=-1.0, group=(na2 // 2) * h * wd_)
            d_score = d_score.view(B, na2, h, wd_)
            delta = rpn[..., na2:].contiguous()                                                          # NHWC [B,h,w,4A]
            tgt = tgt_in.permute(0, 2, 3, 1).contiguous()
            wgt = wgt_in.permute(0, 2, 3, 1).contiguous()
            rpn_l1, d_delta = losses.smooth_l1_loss(delta, tgt, wgt, 3.0, 1.0 / c.rpn_batch_size)
            out['rpn_bbox_loss'] = T.scalar_sum(rpn_l1, 1.0 / B, deterministic=self.deterministic)
            d_rpn = torch.cat([d_score.permute(0, 2, 3, 1), d_delta], 3).to(torch.bfloat16).contiguous()
            # -- proposals and their targets (no gradient: proposal.py:170-173, proposal_target.py:95-97)
            rois, _ = propose_batch(nchw(rpn[..., :na2]), nchw(rpn[..., na2:]), im_info, self.anchors, c.feat_stride,
                                    c.rpn_pre_nms_top_n, c.rpn_post_nms_top_n, c.rpn_nms_thresh, c.rpn_min_size,
                                    im_hw=self.im_hw, softmax_pairs=True)
            N = rois.shape[1]
            # (a step with host-made anchor targets never ran rpn_targets: the sampler advances the step counter itself)
            rois_t, label, bbox_target, bbox_weight, keep = self.roi_targets(rois, gt_boxes, num_gt, advance=early is None)
            R = rois_t.shape[1]
            if keep is not None:    # sampled minibatch: R rows, none of them a key row (plain heads only, check_batch_rois)
                N = R
                br['keep_index'] = out['keep_index'] = keep
                out['proposals'] = br['proposals'] = rois
            br.update(r=r, d_rpn=d_rpn, rois_t=rois_t, label=label, bbox_target=bbox_target, bbox_weight=bbox_weight, N=N, R=R)
            if rpn_bwd_side:
                br['ev'] = torch.cuda.Event()
                br['ev'].record()               # main resumes here (rois and their targets exist); the RPN head's backward follows on this stream
                br['bwd'] = (conv4, r, d_rpn)   # ... once the main stream has made the weight copies it reads (enqueued below)
            if self.metrics is not None:
                # RPNAcc / RPNLogLoss / RPNL1Loss on this stream, BEHIND the event the main stream resumes at: they never lengthen the path to
                # ROI pooling (one image per step: this branch is the longer one), only the RPN head's backward starts two small launches later
                self.metrics.add_rpn(rpn_prob, lbl, rpn_l1)
                br.update(rpn_cls_prob=rpn_prob, rpn_label=lbl, rpn_bbox_loss_map=rpn_l1)
                out['rpn_cls_prob'], out['rpn_label'], out['rpn_bbox_loss_map'] = rpn_prob, lbl, rpn_l1

        def fork(conv4):
            side.wait_stream(main)
            with torch.cuda.stream(side):
                rpn_branch(conv4.to(torch.bfloat16))
        conv5, conv4, saved, _ = self._trunk_forward(data, at_conv4=fork, im_info=im_info)
        # (a float32 trunk -- cfg.trunk_fp32, parity tests -- hands bf16 copies to the bf16 heads and takes their gradients back as float32)
        conv5, conv4 = conv5.to(torch.bfloat16), conv4.to(torch.bfloat16)
        feat = self._conv(conv5, 'conv_new_1', relu=True)
        # W^T / tap-flipped copies of the current weights for every data-gradient product: only the BACKWARD reads them, so they are made
        # here, where the main stream otherwise waits for the proposals (one image: the RPN branch's single-workgroup sort / NMS kernels
        # are the longer path and leave the chip idle)
        self._relayout.run()
        if rpn_bwd_side:
            side.wait_stream(main)
            with torch.cuda.stream(side):       # beside ROI pooling / the 2FC head / the learn-NMS branch (launches of <= 150 workgroups)
                br.update(self._trunk.rpn_backward(*br.pop('bwd')))
            main.wait_event(br['ev'])
        else:
            main.wait_stream(side)
        # the branch's tensors were allocated on the side stream and are consumed on the main one through the backward pass:
        # tell the caching allocator, so that their blocks are not handed out again on the side stream while main still reads them
        if not torch.cuda.is_current_stream_capturing():      # (a capture's private pool keeps its blocks for the graph's lifetime)
            for v in br.values():
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(main)
        rois_t, label, bbox_target, bbox_weight, N, R = (br[k] for k in ('rois_t', 'label', 'bbox_target', 'bbox_weight', 'N', 'R'))
        # (the offset FC's weights are views of the flat buffers that change every step: read when called)
        offset_fc = lambda t0f: ops.gemm_nt(t0f, self.w('offset'), self.b('offset'), out_dtype=torch.float32)
        pooled2, pool_ctx = self.pool.forward([nchw(feat)], rois_t.view(B * R, 5), offset_fc=offset_fc, want_backward=True)
        d_pool, hs = self._head_forward_backward(pooled2, rois_t, N, label, bbox_target, bbox_weight, im_info, gt_boxes, num_gt, out)
        bt = torch.bfloat16
        x2, f1, cls_score, bbox_pred, labels_ohem, weights_ohem = hs
        if self.lnms_only:          # JOINT_TRAINING false: the detector is fixed, the step ends with the learn-NMS head's parameter gradients
            self._bucket_ready('heads')
            out['rois'], out['label'] = rois_t, labels_ohem
            out['bbox_target'], out['bbox_weight'] = bbox_target, weights_ohem
            out['bbox_pred'], out['cls_score'], out['fc_all_2_relu'] = bbox_pred, cls_score, x2
            return out
        # pooling backward -> gradient of conv_new_1_relu (the offset FC's parameter gradients go to this trainer's queues)
        def offset_fc_bwd(t0f, g_trans):
            d_t0, dw, db = T.linear_bwd(t0f, self.w('offset'), g_trans.to(bt), w_t=self.wt('offset'), keep_splits=True, wgrad_to=self._wg('offset'))
            self._add_bgrad('offset', db)
            return d_t0
        d_feat, = self.pool.backward(d_pool, pool_ctx, offset_fc_bwd)
        g = T.relu_bwd(d_feat, feat)
        d_x, dw = T.conv1x1_bwd(conv5, self.w('conv_new_1'), g, w_t=self.wt('conv_new_1'), keep_splits=True, wgrad_to=self._wg('conv_new_1'))
        T.colsum_add(g, *self._bg('conv_new_1'))
        main.wait_stream(side)          # the RPN head's backward (joins the trunk at conv4)
        d_conv4_rpn = br['d_conv4_rpn']
        if self.trunk_fp32:
            d_x, d_conv4_rpn = d_x.float(), d_conv4_rpn.float()
        self._trunk_backward(saved, d_x, {'4b22': d_conv4_rpn})
        out['rois'] = rois_t
        out['label'] = labels_ohem
        out['bbox_target'], out['bbox_weight'] = bbox_target, weights_ohem
        out['bbox_pred'] = bbox_pred
        out['cls_score'] = cls_score
        return out

    def _head_forward_backward(self, pooled2, rois_t, N, label, bbox_target, bbox_weight, im_info, gt_boxes, num_gt, out,
                               key_count=None):
        """2FC head + relation modules + OHEM + losses (+ learn-NMS branch) and their adjoint down to the pooled features.
        pooled2 [B*R, 12544] bf16 ((ph, pw, c) column order), rois_t [B,R,5] with the N non-gt rows first.
        key_count [B] int32 (optional): how many of the first N rows of each image are real proposals (the rest is padding
        of a truncated / short proposal list: no relation keys, label -1, never ranked by the learn-NMS branch).
        Returns (d_pool [B*R,12544] bf16, (x2, f1, cls_score, bbox_pred, labels_ohem, weights_ohem))."""
        c = self.cfg
        B, R = rois_t.shape[0], rois_t.shape[1]
        h = self._box_head.forward(pooled2, rois_t, N, key_count)
        x2, f1, cls_score, bbox_pred = h.x2, h.f1, h.cls_score, h.bbox_pred
        if getattr(c, 'enable_ohem', True):
            labels_ohem, weights_ohem = ops.box_annotator_ohem(cls_score, bbox_pred, label, bbox_target, bbox_weight, c.batch_rois_ohem)
            box_norm = c.batch_rois_ohem
        else:       # ENABLE_OHEM false (symbols/..._learn_nms_1024_...:232-241): every roi counts (padding rows of a short proposal list keep label -1
            labels_ohem, weights_ohem = label, bbox_weight          # and are ignored), the box loss is scaled by 1 / 300 (BATCH_ROIS < 0)
            box_norm = 300
            if getattr(c, 'batch_rois', -1) > 0:                    # a sampled minibatch: 1 / BATCH_ROIS per image (resnet_v1_101_rcnn.py:154-158)
                box_norm = c.batch_rois
        cls_prob, d_cls = losses.softmax_output(cls_score.view(B * R, -1), labels_ohem.reshape(-1), use_ignore=True, ignore_label=-1.0, group=R)
        d_cls = d_cls.view(B, R, -1)
        l1, d_bbox = losses.smooth_l1_loss(bbox_pred, bbox_target, weights_ohem, 1.0, 1.0 / box_norm)
        out['bbox_loss'] = T.scalar_sum(l1, 1.0 / B, deterministic=self.deterministic)
        out['num_ohem'] = T.scalar_sum(labels_ohem, count_nonneg=True, deterministic=self.deterministic)
        if self.metrics is not None:        # RCNNAcc / RCNNLogLoss / RCNNL1Loss (padding rows of a short proposal list have label -1: not counted)
            self.metrics.add_rcnn(cls_prob, labels_ohem.reshape(-1), l1)
            out['cls_prob'], out['bbox_loss_map'] = cls_prob.view(B, R, -1), l1
        d_x2_lnms = None
        if c.learn_nms:     # the learn-NMS head sees the first N (non-gt) rows; its gradient joins cls_score and fc_all_2_relu
            d_cls_l, d_x2_lnms, lo = self._lnms_forward_backward(cls_score[:, :N], bbox_pred[:, :N], rois_t[:, :N].contiguous(),
                                                                 im_info, x2[:, :N], gt_boxes, num_gt, n_valid=key_count, d_cls_out=d_cls)
            if d_cls_l is not None:         # (None: already accumulated into d_cls[:, :N] by relnet_lnms_softmax_bwd)
                d_cls[:, :N] += d_cls_l
            out.update(lo)
        if self.lnms_only:          # every parameter in front of the learn-NMS head is fixed: nothing is differentiated past this point
            return None, (x2, f1, cls_score, bbox_pred, labels_ohem, weights_ohem)
        return self._box_head.backward(h, d_cls, d_bbox, d_x2_lnms), (x2, f1, cls_score, bbox_pred, labels_ohem, weights_ohem)

    def _lnms_forward_backward(self, cls_score, bbox_pred, rois, im_info, feat, gt_boxes, num_gt, n_valid=None, d_cls_out=None):
        """Train branch of the learn-NMS head and its adjoint: learn_nms.LearnNMSTrain.__call__ (arguments and return values there)."""
        return self._lnms(cls_score, bbox_pred, rois, im_info, feat, gt_boxes, num_gt, n_valid=n_valid, d_cls_out=d_cls_out)

    # ---- checkpoint view -----------------------------------------------------------------------------------
    def export_params(self):
        """The trainable parameters back under the reference's names and layouts (fp32, on the host): convolution
        weights [O,I,kh,kw] with the folded BatchNorm scale divided out again, fc_new_1 / roi_pool_fc1 columns back in
        (c, ph, pw) order, the fused RPN / query|key / cls|bbox matrices split.  Frozen tensors are not returned."""
        out = {}
        wv = lambda n: self.W.view(self.W.master, n).detach().cpu()
        bv = lambda n: self.Bv.view(self.Bv.master, n).detach().cpu()

        def unpack(w2d, k):
            o = w2d.shape[0]
            return w2d.view(o, k, k, -1).permute(0, 3, 1, 2).contiguous()

        for name in self.W.slices:
            if name in self.bn_scale:                                   # res3..res5 convolutions
                out[name + '_weight'] = unpack(wv(name) / self.bn_scale[name].cpu().view(-1, 1), self.ksize[name])
            elif name.startswith('fpn_') or name in ('rpn_conv_3x3', 'conv_new_1') or name.endswith('_offset'):
                out[name + '_weight'] = unpack(wv(name), self.ksize.get(name, 1)); out[name + '_bias'] = bv(name)
        if not self.fpn:
            w, b = wv('rpn_out'), bv('rpn_out')
            out['rpn_cls_score_weight'], out['rpn_bbox_pred_weight'] = unpack(w[:self.na2], 1), unpack(w[self.na2:], 1)
            out['rpn_cls_score_bias'], out['rpn_bbox_pred_bias'] = b[:self.na2].clone(), b[self.na2:].clone()
        inv = torch.empty_like(self.fc1_perm); inv[self.fc1_perm] = torch.arange(len(self.fc1_perm))
        n1, n2 = self.fc_names
        out[n1 + '_weight'], out[n1 + '_bias'] = wv('fc_new_1')[:, inv].contiguous(), bv('fc_new_1')
        out[n2 + '_weight'], out[n2 + '_bias'] = wv('fc_new_2').clone(), bv('fc_new_2')
        nc = self.num_classes
        out['cls_score_weight'], out['bbox_pred_weight'] = wv('cls_bbox')[:nc].clone(), wv('cls_bbox')[nc:].clone()
        out['cls_score_bias'], out['bbox_pred_bias'] = bv('cls_bbox')[:nc].clone(), bv('cls_bbox')[nc:].clone()
        mods = ([('', i) for i in (1, 2)] if self.relation else []) + ([('nms_', 1)] if self.cfg.learn_nms else [])
        for pre, i in mods:
            qk, bq = wv('%sqk_%d' % (pre, i)), bv('%sqk_%d' % (pre, i))
            h = qk.shape[0] // 2
            out['%squery_%d_weight' % (pre, i)], out['%skey_%d_weight' % (pre, i)] = qk[:h].clone(), qk[h:].clone()
            out['%squery_%d_bias' % (pre, i)], out['%skey_%d_bias' % (pre, i)] = bq[:h].clone(), bq[h:].clone()
            wo = wv('%slinear_out_%d' % (pre, i))
            out['%slinear_out_%d_weight' % (pre, i)] = wo.reshape(wo.shape[0], wo.shape[1], 1, 1).clone()
            out['%slinear_out_%d_bias' % (pre, i)] = bv('%slinear_out_%d' % (pre, i))
            out['%spair_pos_fc1_%d_weight' % (pre, i)] = wv('%spair_pos_fc1_%d' % (pre, i)).clone()
            out['%spair_pos_fc1_%d_bias' % (pre, i)] = bv('%spair_pos_fc1_%d' % (pre, i))
        if self.cfg.learn_nms:
            for n in ('nms_rank', 'roi_feat_embedding', 'nms_logit'):
                out[n + '_weight'], out[n + '_bias'] = wv(n).clone(), bv(n)
        if self.cfg.dcn:
            out['offset_weight'], out['offset_bias'] = wv('offset')[:, inv].contiguous(), bv('offset')
        return out

    def checkpoint_params(self):
        """(arg_params, aux_params) as MXNet's Module hands them to the epoch-end callback (core/module.py fit ->
        callback.do_checkpoint): every trainable tensor (export_params) plus the frozen ones under `arg`, the BatchNorm
        running statistics under `aux`.  `checkpoint.do_checkpoint(prefix, means, stds)` turns them into the reference's
        `.params` file incl. the de-normalised `bbox_pred_*_test` pair (core/callback.py:54-61)."""
        arg = self.export_params()
        aux = {}
        for k, v in self._fixed_src.items():
            (aux if 'moving_' in k else arg).setdefault(k, v.clone())
        return arg, aux

    def save_checkpoint(self, prefix, epoch):
        """`<prefix>-<epoch+1:04d>.params` exactly as train_end2end.py:149-152 + core/callback.py:54-61 write it
        (means / stds tiled over the regression classes: 2 when class agnostic)."""
        from . import checkpoint as ck
        c = self.cfg
        reps = 2 if getattr(c, 'class_agnostic', True) else c.num_classes
        means, stds = list(c.bbox_means) * reps, list(c.bbox_stds) * reps
        arg, aux = self.checkpoint_params()
        return ck.do_checkpoint(prefix, means, stds)(epoch, None, arg, aux)

    # ---- optimizer ----------------------------------------------------------------------------------------
    def _grad_buckets(self):
        """Weight-gradient buckets in buffer (= forward) order: res3 | res4 (first half) | res4 (second half) | res5 | everything after
        the trunk (RPN, conv_new_1 / FPN neck, 2FC + relation + learn-NMS heads).  The backward pass completes them last to first.
        res4's 104 MB are two buckets (cut at unit b11): its second half travels while the first half is still being differentiated,
        and what is left exposed after the last backward kernel is res3 (4.9 MB) plus the tail of a 47 MB message instead of 104 MB."""
        if getattr(self, '_buckets', None) is None and self.lnms_only:
            # (learn-NMS-only step: one bucket -- only the head's tail of the buffer ever holds a non-zero gradient)
            self._bucket_cuts, self._bucket_names, self._unit_bucket = [0, self.W.size], ('heads',), {}
            self._buckets = D.BucketedAllReduce(self.W.grad, self._bucket_cuts)
        if getattr(self, '_buckets', None) is None:
            trunk = [n for n in self.W.slices if n in self.bn_scale]            # BN-folded res3..res5 convolutions
            first = lambda pre: min(self.W.slices[n][0] for n in trunk if n.startswith(pre))
            trunk_end = max(self.W.slices[n][0] + (int(np.prod(self.W.slices[n][1])) + 63) // 64 * 64 for n in trunk)
            res4 = [u[1] for u in self.units if u[0] == 4]
            half = res4[len(res4) // 2]                                        # '4b11' of 4a, 4b1 .. 4b22
            cuts = [0, first('res4'), first('res' + half + '_'), first('res5'), trunk_end, self.W.size]
            self._bucket_names = ('res3', 'res4_lo', 'res4_hi', 'res5', 'heads')
            if self.res2_trainable:         # conv1 (when trainable) + res2 in front of res3: bucket 0, the last one the backward pass announces
                cuts = [0, first('res3')] + cuts[1:]
                self._bucket_names = ('res2',) + self._bucket_names
            assert cuts == sorted(set(cuts)), cuts
            self._bucket_cuts = cuts
            self._unit_bucket = {}
            hi = False
            for u in self.units:
                if u[0] < 3 and not self.res2_trainable:
                    continue
                if u[0] == 4:
                    hi = hi or (u[1] == half)
                    self._unit_bucket[u[1]] = 'res4_hi' if hi else 'res4_lo'
                else:
                    self._unit_bucket[u[1]] = 'res%d' % u[0]
            self._buckets = D.BucketedAllReduce(self.W.grad, cuts)
        return self._buckets

    def _bucket_ready(self, *names):
        """Called by the backward pass when the last gradient of a bucket (or of several at once) has been queued (no-op on one rank)."""
        self._flush_wgrads()         # the bucket is complete only once its queued gradient work has been launched
        bk = self._grad_buckets()
        idxs = [self._bucket_names.index(n) for n in names]
        cut = getattr(self, '_capture_cut', None)
        if cut is not None:          # CapturedStep: close the current hipGraph here; the collective(s) go between two graphs
            cut(idxs[0] if len(idxs) == 1 else tuple(idxs))
            return
        for idx in idxs:
            bk.ready(idx)

    def all_reduce(self, wait=True):
        """Summed all-reduce of the gradients over RCCL (MXNet kvstore 'device' + rescale_grad 1.0 semantics): the weight
        buckets -- those the backward pass has not already launched -- and the 0.1 MB bias buffer.  wait=False only LAUNCHES what is
        missing: `update()` then waits bucket by bucket, in the order they were launched, and runs SGD on a bucket as soon as ITS
        sum has landed -- the optimizer of the heads / res5 buckets overlaps the all-reduce of res4 / res3 still in flight."""
        bk = self._grad_buckets()
        if not wait and bk.active():
            order = bk.launch_rest()
            self._bias_work = D.all_reduce_async(self.Bv.grad)
            return order
        order = bk.finish()
        all_reduce_sum(self.Bv.grad)
        self._bias_work = None
        return order

    def _trainable_ranges(self, buf):
        """Contiguous element ranges of a flat buffer that hold trainable slices (everything, unless network.FIXED_PARAMS fixes some)."""
        if not self.frozen_names:
            return [(0, buf.size)]
        key = id(buf)
        cache = self.__dict__.setdefault('_range_cache', {})
        if key not in cache:
            rs = []
            for n, (off, shape) in sorted(buf.slices.items(), key=lambda kv: kv[1][0]):
                if n in self.frozen_names:
                    continue
                end = off + (int(np.prod(shape)) + 63) // 64 * 64
                if rs and rs[-1][1] == off:
                    rs[-1] = (rs[-1][0], end)
                else:
                    rs.append((off, end))
            cache[key] = rs
        return cache[key]

    def _sgd(self, buf, lo, hi, lr, wd, bf16=True, guard=None):
        for a, b_ in self._trainable_ranges(buf):          # (fixed parameters: neither gradient step nor weight decay nor momentum)
            l, h = max(lo, a), min(hi, b_)
            if h > l and guard is None:
                T.sgd_update(buf.master[l:h], buf.mom[l:h], buf.grad[l:h], lr, self.cfg.momentum, wd, 1.0,
                             w_bf16=buf.work[l:h] if bf16 else None)
            elif h > l:
                T.sgd_update_guarded(buf.master[l:h], buf.mom[l:h], buf.grad[l:h], lr, guard.state, self.cfg.momentum, wd, 1.0,
                                     clip_gradient=-1.0 if guard.clip_gradient is None else guard.clip_gradient,
                                     w_bf16=buf.work[l:h] if bf16 else None)

    def _grad_views(self, buf, lo, hi):
        """The trainable gradient ranges of a flat buffer inside [lo, hi): what `_sgd` updates there (frozen slices excluded, the
        lr_mult tail included -- lr_mult scales the step, not the gradient)."""
        return [buf.grad[max(lo, a):min(hi, b_)] for a, b_ in self._trainable_ranges(buf) if min(hi, b_) > max(lo, a)]

    def update(self, lr=None):
        """mx.optimizer.SGD over the flat buffers.  One rank (or everything already waited for): one launch for the weights, one for
        the biases.  With bucket all-reduces in flight (all_reduce(wait=False)): per bucket, in launch order, wait + SGD on its slice.

        With a guard (`self.guard`, a GradGuard) the gradient statistics take SGD's place in that loop -- a bucket's are launched right
        after its wait and run while later buckets are still in flight, the biases' after the bias wait -- then ONE decide launch, then
        the guarded SGD launches.  The decision needs every gradient, so with a guard SGD starts only after the last collective has
        landed: that is inherent in a global norm.  On one rank the guard adds three launches (statistics of the weights, of the
        biases, decide; one more statistics launch per 16 trainable ranges of a buffer beyond the first 16).  `step_count` advances on
        a skipped step too: the host does not know, and the LR schedule stays a function of the call count."""
        c = self.cfg
        lr = c.lr if lr is None else lr
        W, Bv = self.W, self.Bv
        guard = self.guard
        wo, bo, mult = self.lr_mult_tail if self.lr_mult_tail is not None else (W.size, Bv.size, 1.0)
        bk = self._grad_buckets()
        pending = []
        if bk.active():
            # every bucket must have been exchanged before its slice is updated: a caller that skipped all_reduce() (or whose backward
            # pass announced only some buckets) gets the missing collectives launched here instead of a silently local update
            if not bk.exchanged:                    # (exchanged: all_reduce(wait=True) already summed this pass's gradients)
                if len(bk.done) < bk.n:
                    bk.launch_rest()
                if getattr(self, '_bias_work', None) is None:
                    self._bias_work = D.all_reduce_async(self.Bv.grad)
                assert len(bk.done) == bk.n
            pending = bk.pending_order()
        self.update_order = []                      # (bucket index, its collective had completed when SGD was queued) -- test hook
        ranges = [(self._bucket_cuts[i], self._bucket_cuts[i + 1], i) for i in pending] if pending else [(0, W.size, None)]
        timing = getattr(self, 'comm_timing', None)   # list (bench.py --gpus N): per bucket, (name, event before the wait, event after it)
        if guard is not None:
            guard.bind(W.grad.device)
            plan = [self._grad_views(W, lo, hi) for lo, hi, _ in ranges] + [self._grad_views(Bv, 0, Bv.size)]
            guard.begin(sum(T.grad_stats_slots([v.numel() for v in vs[k:k + T.GUARD_MAX_RANGES]])
                            for vs in plan for k in range(0, len(vs), T.GUARD_MAX_RANGES)))
        for lo, hi, i in ranges:
            if i is not None:
                self.update_order.append((i, bk.is_completed(i)))
                if timing is not None:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                bk.wait(i)
                if timing is not None:
                    e1.record()
                    timing.append((self._bucket_names[i], e0, e1))
            if guard is not None:
                guard.stats(self._grad_views(W, lo, hi))
                continue
            # parameters with lr_mult != 1 (DCN `offset` FC) sit at the tail of both flat buffers
            self._sgd(W, lo, min(hi, wo), lr, c.wd)
            self._sgd(W, max(lo, wo), hi, lr * mult, c.wd)
        if pending:
            bk.clear()
        if getattr(self, '_bias_work', None) is not None:
            if timing is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            D.wait_work(self._bias_work, self.Bv.grad)
            if timing is not None:
                e1.record()
                timing.append(('biases', e0, e1))
            self._bias_work = None
        if guard is not None:
            guard.stats(self._grad_views(Bv, 0, Bv.size))
            guard.decide()
            for lo, hi, _ in ranges:
                self._sgd(W, lo, min(hi, wo), lr, c.wd, guard=guard)
                self._sgd(W, max(lo, wo), hi, lr * mult, c.wd, guard=guard)
        self._sgd(Bv, 0, bo, lr, 0.0, bf16=False, guard=guard)
        self._sgd(Bv, bo, Bv.size, lr * mult, 0.0, bf16=False, guard=guard)
        self.step_count += 1

    def comm_report(self, steps):
        """Exposed communication of the steps since `comm_timing = []` was set: per gradient bucket, the time the COMPUTE stream sat
        in that bucket's wait (event before / after the wait, both on the compute stream: zero when the collective had finished under
        the backward pass), averaged over `steps`; plus their sum per step.  Call after a device synchronisation."""
        per = {}
        for name, e0, e1 in (getattr(self, 'comm_timing', None) or []):
            per[name] = per.get(name, 0.0) + e0.elapsed_time(e1)
        per = {k: v / max(steps, 1) for k, v in per.items()}
        mb = {n: 4e-6 * (self._bucket_cuts[i + 1] - self._bucket_cuts[i]) for i, n in enumerate(self._bucket_names)}
        mb['biases'] = 4e-6 * self.Bv.size
        return {'exposed_wait_ms_per_step': {k: round(v, 4) for k, v in per.items()},
                'exposed_comm_ms_per_step': round(sum(per.values()), 4),
                'bucket_megabytes': {k: round(v, 1) for k, v in mb.items()},
                'how': 'HIP events on the compute stream around each bucket\'s wait in Trainer.update(): the time the optimizer was held up by a '
                       'collective still in flight (0 = fully hidden under the backward pass)'}

    def step(self, *batch, **kw):
        out = self.forward_backward(*batch, **kw)
        self.all_reduce(wait=False)
        self.update()
        return out


class CapturedStep(object):
    """forward + backward of a trainer captured as a CHAIN of hipGraphs, cut where a gradient bucket completes
    (heads | res5 | res4 | res3, the order the backward pass finishes them): on replay every bucket's summed all-reduce is
    issued from the host BETWEEN two graph launches, on the communication stream, and runs under the next segment's kernels --
    the overlap of dist.BucketedAllReduce without the ~10 ms of eager Python launches per step, and without capturing the
    collective itself (a captured RCCL call would pin the communicator's buffers into the graph).
    The reference overlaps nothing: kvstore push / pull runs after the whole backward pass (core/module.py:569-591).

        step = CapturedStep(trainer, batch)          # one eager warm-up must have run before (kernel attributes, caches)
        out = step.replay(); trainer.all_reduce(); trainer.update()
    """

    def __init__(self, trainer, batch, kwargs=None, segments=None):
        """segments: True = cut at every gradient bucket; None (default) = cut only when there is somebody to exchange the buckets with
        (a process group of more than one rank) -- on one rank the whole pass is ONE hipGraph (round 6: five graph launches and their seams
        less per step)."""
        self.tr = trainer
        do_cut = trainer._grad_buckets().active() if segments is None else bool(segments)
        if trainer.step_count == 0:              # kernel attributes (hipFuncSetAttribute), allocator pools and caches must exist before a capture
            with torch.no_grad():
                trainer.forward_backward(*batch, **(kwargs or {}))
                trainer.all_reduce()             # completes the bucket exchanges that pass announced (every rank does the same)
            torch.cuda.synchronize()
        self.segments = []                       # [(hipGraph, bucket index or None)]
        pool = torch.cuda.graph_pool_handle()    # one private pool: tensors made in one segment stay valid in the next ones
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        cur = [None]

        def begin():
            cur[0] = torch.cuda.CUDAGraph()
            # thread_local: with a process group up, RCCL's watchdog thread polls events while this thread captures; in the default 'global'
            # capture mode a CUDA call from ANOTHER thread invalidates the capture (never an issue on one rank / over gloo)
            cur[0].capture_begin(pool=pool, capture_error_mode='thread_local')

        def cut(idx):
            if not do_cut:               # one rank: nothing is exchanged between the segments, keep capturing into the same graph
                return
            cur[0].capture_end()
            self.segments.append((cur[0], idx))
            if idx == 0 or (isinstance(idx, tuple) and 0 in idx):   # bucket 0 (res3) is announced by the last kernel of the backward pass: nothing follows, so no
                cur[0] = None            # further capture is opened (an empty hipGraph used to be captured here and warned about on stderr)
            else:
                begin()

        torch.cuda.synchronize()
        with torch.cuda.stream(side), torch.no_grad():
            begin()
            trainer._capture_cut = cut
            import warnings
            try:
                self.out = trainer.forward_backward(*batch, **(kwargs or {}))
            except BaseException:
                trainer._capture_cut = None
                try:                              # leave capture mode, but let the ORIGINAL error propagate
                    if cur[0] is not None:
                        cur[0].capture_end()
                except Exception:
                    pass
                raise
            trainer._capture_cut = None
            if cur[0] is not None:       # (a trainer whose backward did not end with bucket 0: keep its tail)
                with warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter('always')
                    cur[0].capture_end()
                if not any('Graph is empty' in str(w.message) for w in caught):
                    self.segments.append((cur[0], None))
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def replay(self):
        """Launch the segments in order; after each one, announce its bucket (asynchronous all-reduce on >1 rank)."""
        bk = self.tr._grad_buckets()
        bk.reset()
        for graph, idx in self.segments:
            graph.replay()
            for i in (() if idx is None else idx if isinstance(idx, tuple) else (idx,)):
                bk.ready(i)
        return self.out


class FPNTrainer(Trainer):
    """Training step of the FPN relation graphs (BASELINE configs[4]; symbols/resnet_v1_101_rcnn_fpn_attention_1024_
    pairwise_position_multi_head_16_learn_nms.py, get_symbol_rcnn train branch :1040-1200): proposals are an input
    (HAS_RPN: false, TOP_ROIS 1000), their labels / targets come from proposal_target-style sampling with the gt rows
    appended, rois are dispatched to the pyramid levels (core/rcnn.py:53-74) and pooled from fpn_ft4..ft32.

    Row order: the reference keeps a level-major order over ALL rows and selects the relation keys with `nongt_index`
    (:881-885, 931); here the non-gt rows are dispatched first and the gt rows after them, so the keys are the first N
    rows -- the same set of keys, and every per-roi output is mapped back through `perm`."""

    scales = (1 / 4.0, 1 / 8.0, 1 / 16.0, 1 / 32.0)

    def __init__(self, params, cfg=None, device='cuda', metrics=None, guard=None):
        cfg = cfg or TrainConfig()
        cfg.fpn = True
        check_deterministic(cfg)        # (before anything is built: the FPN pooling backward has no ordered form)
        Trainer.__init__(self, params, cfg, device, im_hw=None, metrics=metrics, guard=guard)

    def _forward_backward_impl(self, data, im_info, gt_boxes, proposals, num_gt=None, num_proposals=None):
        """data [B,3,H,W] (H, W multiples of 32), proposals [B,N,4] fp32, gt_boxes [B,G,5]; num_proposals [B] int32
        (optional): real rows of `proposals` per image -- the reference hands every image its own roi count
        (core/rcnn.py:128-146, TOP_ROIS truncation only); a batched step pads to a common N and the padded rows are
        taken out on the device: zero box, label -1, zero weights (relnet_proposal_target_ex), moved behind the real rows by
        the level dispatch, no relation keys (key_count), never ranked by the learn-NMS branch."""
        c = self.cfg
        B, N = proposals.shape[:2]
        if any(n % 32 for n in ops.image_hw(data)):
            raise ValueError("FPN images must be padded to IMAGE_STRIDE 32, got %s" % (tuple(data.shape),))
        self._grad_buckets().reset()
        self.W.grad.zero_(); self.Bv.grad.zero_()
        self._relayout.run()            # W^T / tap-flipped copies of the current weights for every data-gradient product
        self._fragpack.run()            # ... and the fragment-order copies the chain kernels of the forward read
        out = {}
        conv5, conv4, saved, ends = self._trunk_forward(data, im_info=im_info)
        feats, neck_ctx = self._trunk.neck_forward(ends)      # 1x1 laterals (+bias), nearest 2x upsampling + sum, 3x3 output convs
        # ---- rois: labels / targets, then level dispatch (non-gt rows first, gt rows after)
        rois5 = torch.cat([torch.zeros((B, N, 1), device=proposals.device), proposals], 2)
        rois5[:, :, 0] = torch.arange(B, device=proposals.device, dtype=torch.float32).view(B, 1)
        # (this trainer never runs rpn_targets: a sampled minibatch advances the device step counter itself)
        rois_t, label, bbox_target, bbox_weight, keep = self.roi_targets(rois5.contiguous(), gt_boxes, num_gt, num_rois=num_proposals, advance=True)
        R = rois_t.shape[1]
        key_count = None
        if keep is not None:        # sampled minibatch (resnet_v1_101_rcnn_fpn.py:1172-1179): R rows drawn from the num_proposals real rows + the gt
            N = R                   # rows -- no padded row among them, no key rows (plain heads only, check_batch_rois): one dispatch
            rois_s, level, pa, _ = ops.fpn_roi_dispatch(rois_t)
            perm = pa.long()
            out['keep_index'] = keep
        else:
            if num_proposals is not None:
                ra, la, pa, _, key_count = ops.fpn_roi_dispatch(rois_t[:, :N].contiguous(), n_valid=num_proposals)
            else:
                ra, la, pa, _ = ops.fpn_roi_dispatch(rois_t[:, :N].contiguous())
            rb, lb, pb, _ = ops.fpn_roi_dispatch(rois_t[:, N:].contiguous())
            rois_s = torch.cat([ra, rb], 1).contiguous()
            level = torch.cat([la, lb], 1).contiguous()
            perm = torch.cat([pa, pb + N], 1).long()
        gat = lambda t: torch.gather(t, 1, perm.view(B, R, *([1] * (t.dim() - 2))).expand(B, R, *t.shape[2:]))
        label, bbox_target, bbox_weight = gat(label), gat(bbox_target).contiguous(), gat(bbox_weight).contiguous()
        lv = [feats[lvl].permute(0, 3, 1, 2) for lvl in (4, 8, 16, 32)]
        pooled2, pool_ctx = self.pool.forward(lv, rois_s.view(B * R, 5), level.view(-1), want_backward=True)
        d_pool, hs = self._head_forward_backward(pooled2, rois_s, N, label.contiguous(), bbox_target, bbox_weight, im_info,
                                                 gt_boxes, num_gt, out, key_count=key_count)
        x2, f1, cls_score, bbox_pred, labels_ohem, weights_ohem = hs
        # ---- pooling backward into the four pyramid maps
        d_feats = dict(zip((4, 8, 16, 32), self.pool.backward(d_pool, pool_ctx)))
        d_c5, inject = self._trunk.neck_backward(neck_ctx, d_feats)
        self._trunk_backward(saved, d_c5, inject)
        out.update(rois=rois_s, perm=perm, roi_level=level, label=labels_ohem, bbox_target=bbox_target, bbox_weight=weights_ohem,
                   bbox_pred=bbox_pred, cls_score=cls_score)
        out['intermediates'] = dict(feats=feats, pooled=pooled2)        # forward values for the stage-wise parity test
        return out


def assign_anchor(feat_hw, gt_boxes, im_hw, cfg, seed=0, allowed_border=0):
    """Host-side RPN label preparation (the reference does this in its data loader: lib/rpn/rpn.py:80-244).
    gt_boxes [G,5] numpy; returns label [A*h*w] ((a,y,x) order), bbox_target [4A,h,w], bbox_weight [4A,h,w]."""
    rng = np.random.RandomState(seed)
    base = generate_anchors(cfg.feat_stride, cfg.anchor_ratios, cfg.anchor_scales).astype(np.float64)
    A = base.shape[0]
    fh, fw = feat_hw
    sx, sy = np.meshgrid(np.arange(fw) * cfg.feat_stride, np.arange(fh) * cfg.feat_stride)
    shifts = np.stack([sx.ravel(), sy.ravel(), sx.ravel(), sy.ravel()], 1)
    anchors = (base[None] + shifts[:, None]).reshape(-1, 4)                  # (y, x, a) major -> K*A rows
    total = anchors.shape[0]
    inside = np.where((anchors[:, 0] >= -allowed_border) & (anchors[:, 1] >= -allowed_border) &
                      (anchors[:, 2] < im_hw[1] + allowed_border) & (anchors[:, 3] < im_hw[0] + allowed_border))[0]
    a = anchors[inside]
    labels = np.full(len(inside), -1, np.float32)
    targets = np.zeros((len(inside), 4), np.float32)
    if gt_boxes.size > 0:
        g = gt_boxes[:, :4].astype(np.float64)
        iw = np.minimum(a[:, None, 2], g[None, :, 2]) - np.maximum(a[:, None, 0], g[None, :, 0]) + 1
        ih = np.minimum(a[:, None, 3], g[None, :, 3]) - np.maximum(a[:, None, 1], g[None, :, 1]) + 1
        inter = np.clip(iw, 0, None) * np.clip(ih, 0, None)
        aa = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
        ga = (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)
        ov = inter / (aa[:, None] + ga[None] - inter)
        amax = ov.argmax(1)
        mx = ov[np.arange(len(a)), amax]
        gt_best = ov.max(0)
        labels[mx < 0.3] = 0                                                  # RPN_NEGATIVE_OVERLAP (no clobber)
        labels[np.where(ov == gt_best[None])[0]] = 1
        labels[mx >= 0.7] = 1                                                 # RPN_POSITIVE_OVERLAP
        # bbox_transform(anchors, matched gt), lib/bbox/bbox_transform.py:74-100
        gm = g[amax]
        ew, eh = a[:, 2] - a[:, 0] + 1, a[:, 3] - a[:, 1] + 1
        ecx, ecy = a[:, 0] + 0.5 * (ew - 1), a[:, 1] + 0.5 * (eh - 1)
        gw_, gh_ = gm[:, 2] - gm[:, 0] + 1, gm[:, 3] - gm[:, 1] + 1
        gcx, gcy = gm[:, 0] + 0.5 * (gw_ - 1), gm[:, 1] + 0.5 * (gh_ - 1)
        targets[:] = np.stack([(gcx - ecx) / (ew + 1e-14), (gcy - ecy) / (eh + 1e-14), np.log(gw_ / ew), np.log(gh_ / eh)], 1)
    else:
        labels[:] = 0
    num_fg = int(0.5 * cfg.rpn_batch_size)
    fg = np.where(labels == 1)[0]
    if len(fg) > num_fg:
        labels[rng.choice(fg, len(fg) - num_fg, replace=False)] = -1
    bg = np.where(labels == 0)[0]
    num_bg = cfg.rpn_batch_size - int((labels == 1).sum())
    if len(bg) > num_bg:
        labels[rng.choice(bg, len(bg) - num_bg, replace=False)] = -1
    weights = np.zeros((len(inside), 4), np.float32)
    weights[labels == 1] = 1.0
    L = np.full(total, -1, np.float32); L[inside] = labels
    Tg = np.zeros((total, 4), np.float32); Tg[inside] = targets
    Wg = np.zeros((total, 4), np.float32); Wg[inside] = weights
    L = L.reshape(fh, fw, A).transpose(2, 0, 1).reshape(-1)
    Tg = Tg.reshape(fh, fw, A * 4).transpose(2, 0, 1)
    Wg = Wg.reshape(fh, fw, A * 4).transpose(2, 0, 1)
    return L, Tg, Wg
