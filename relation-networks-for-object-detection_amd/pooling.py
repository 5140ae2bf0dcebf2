"""The ROI pooling stage of the four graphs (Detector, FPNDetector, Trainer, FPNTrainer): 7x7 features of every roi, from one map
(C4: conv_new_1_relu at 1 / feat_stride) or from the pyramid level the roi was dispatched to, and the adjoint of that.

This is the one place that knows which operator pools (ROIPooling as in the reference graphs, SYM_REL:252-253; ROIAlign with
cfg.roi_align; the two-pass deformable PSROI pooling of the DCN graph, SYM_DCN_RELNMS:1073-1080), that the maps are logical NCHW views
of NHWC memory, that fc_new_1 / roi_pool_fc1 take their columns in (ph, pw, c) order, and what each operator's backward keeps.
"""
import torch

from . import ops

def check_pooling(cfg):
    """cfg.roi_align together with cfg.dcn: the DCN graph pools with deformable PSROI pooling (SYM_DCN_RELNMS:1073-1080), there is no
    ROIAlign in it to switch to -- refused rather than silently ignored."""
    if getattr(cfg, 'roi_align', False) and getattr(cfg, 'dcn', False):
        raise ValueError("roi_align and dcn cannot be combined: the DCN graph pools with deformable PSROI pooling")


class RoiPooling(object):
    def __init__(self, cfg, scales, deterministic=False):
        """scales: the spatial scale of every map `forward` will be given (one for the C4 graphs, four for the pyramid).
        deterministic: the ordered form of the ROIPooling adjoint (ops.roi_pool_bwd(deterministic=True))."""
        check_pooling(cfg)
        self.cfg, self.scales, self.deterministic = cfg, tuple(scales), bool(deterministic)
        self.kind = 'dcn' if getattr(cfg, 'dcn', False) else 'align' if getattr(cfg, 'roi_align', False) else 'pool'
        # what has no kernel (the trainers refuse the same by name first: train.check_deterministic)
        assert len(self.scales) == 1 or self.kind != 'dcn', "deformable PSROI pooling reads one map"
        assert len(self.scales) == 1 or not self.deterministic, "the pyramid ROIPooling adjoint has no ordered form"
        assert self.kind == 'pool' or not self.deterministic, "only the ROIPooling adjoint has an ordered form"

    def _deform(self, feat, rois5, trans):
        c = self.cfg
        return ops.deformable_psroi_pool(feat, rois5, trans, self.scales[0], feat.shape[1], 1, 7, 7, c.dcn_sample_per_part,
                                         0.0 if trans is None else c.dcn_trans_std, trans is None, channels_last_out=True)

    def _deform_bwd(self, grad, feat, rois5, trans):
        c = self.cfg
        return ops.deformable_psroi_pool_bwd(grad, feat, rois5, trans, self.scales[0], feat.shape[1], 1, 7, 7, c.dcn_sample_per_part,
                                             0.0 if trans is None else c.dcn_trans_std, trans is None)

    def forward(self, maps, rois5, roi_level=None, offset_fc=None, want_backward=False):
        """maps: list of logical [B,C,H,W] tensors (any strides), rois5 [R,5], roi_level [R] int32 with more than one map.
        offset_fc (DCN): t0f [R, 49 C] -> the offsets, 2 * 49 per roi (SYM_DCN_RELNMS:1075).
        -> pooled2 [R, 49 C] in (ph, pw, c) column order (no copy); with want_backward also the context `backward` takes."""
        assert len(maps) == len(self.scales)
        R = rois5.shape[0]
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(R, -1)               # (ph, pw, c) order, no copy
        ctx = dict(maps=maps, rois=rois5, level=roi_level)
        if self.kind == 'dcn':
            t0f = flat(self._deform(maps[0], rois5, None))
            trans = offset_fc(t0f).view(R, 2, 7, 7)
            pooled = self._deform(maps[0], rois5, trans)
            ctx.update(t0f=t0f, trans=trans)
        elif self.kind == 'align':     # (one map, no level table: the single-map case of the levels kernels)
            pooled = ops.roi_align_fpn(maps, self.scales, rois5, roi_level, (7, 7), self.cfg.roi_align_sampling, channels_last_out=True)
        else:
            if len(maps) == 1:
                pooled = ops.roi_pool(maps[0], rois5, (7, 7), self.scales[0], channels_last_out=True, want_argmax=want_backward)
            else:
                pooled = ops.roi_pool_fpn(maps, self.scales, rois5, roi_level, (7, 7), channels_last_out=True, want_argmax=want_backward)
            if want_backward:
                pooled, ctx['argmax'] = pooled
        return (flat(pooled), ctx) if want_backward else flat(pooled)

    def backward(self, d_pool, ctx, offset_fc_bwd=None):
        """d_pool [R, 49 C] bf16, ctx from forward(want_backward=True).  offset_fc_bwd (DCN): (t0f, gradient of the offsets [R, 98] fp32)
        -> gradient of t0f; it owns the offset FC's parameter gradients.  -> one NHWC bf16 gradient per map, the layout the trunk's and
        the neck's backward take (the kernels accumulate in fp32, logical NCHW over NHWC memory: one conversion pass)."""
        return [g.permute(0, 2, 3, 1).to(torch.bfloat16) for g in self.backward_f32(d_pool, ctx, offset_fc_bwd)]

    def backward_f32(self, d_pool, ctx, offset_fc_bwd=None):
        """`backward` before its conversion: the fp32 gradients as the kernels leave them, logical [B,C,H,W] over NHWC memory."""
        maps, rois5, level = ctx['maps'], ctx['rois'], ctx['level']
        R = rois5.shape[0]
        unflat = lambda t: t.view(R, 7, 7, -1).permute(0, 3, 1, 2)
        shapes = [tuple(t.shape) for t in maps]
        if self.kind == 'dcn':
            gd1, g_trans = self._deform_bwd(unflat(d_pool), maps[0], rois5, ctx['trans'])
            d_t0 = offset_fc_bwd(ctx['t0f'], g_trans.view(R, -1))
            gd2, _ = self._deform_bwd(unflat(d_t0), maps[0], rois5, None)
            return [gd1 + gd2]
        if self.kind == 'align':
            return ops.roi_align_fpn_bwd(unflat(d_pool), rois5, level, shapes, self.scales, self.cfg.roi_align_sampling, channels_last=True)
        if len(maps) == 1:
            return [ops.roi_pool_bwd(unflat(d_pool), ctx['argmax'], rois5, shapes[0], channels_last=True,
                                     deterministic=self.deterministic, spatial_scale=self.scales[0])]
        return ops.roi_pool_fpn_bwd(unflat(d_pool), ctx['argmax'], rois5, level, shapes, channels_last=True)
