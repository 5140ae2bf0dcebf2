"""Host side of the learned duplicate-removal head: the test branch (LearnNMS) and the train branch with its adjoint (LearnNMSTrain).

LearnNMS mirrors relation_rcnn/operator_py/learn_nms.py (LearnNmsOperator.forward :238-401) and the merge of
symbols/..._learn_nms.py:553-560, batched over B images, with no host synchronisation: the
reference's numpy class filtering (:296-303) becomes an on-device valid-class predicate.
LearnNMSTrain is symbols/..._learn_nms.py:424-551 on a Trainer's parameters.  Both rank through `rank_stage`; every kernel is reached
through its front end in ops / train_ops / losses.
"""
import collections
from types import SimpleNamespace

import torch

from . import ops, losses, train_ops as T
from .relation import pack_pair_pos, _module_forward, attention_module_backward, GradSink


def rank_embedding(rank_dim, feat_dim=1024, wave_length=1000.0):
    """learn_nms.py:129-140 in float32 (MXNet arange / broadcast_power / broadcast_div), sin/cos
    correctly rounded.  A constant of the network -> evaluated once on the host."""
    r = torch.arange(0, rank_dim, dtype=torch.float32)[:, None]
    k = torch.arange(0, feat_dim // 2, dtype=torch.float32)
    dim = torch.pow(torch.tensor(float(wave_length), dtype=torch.float32), torch.tensor(2.0 / feat_dim, dtype=torch.float32) * k)[None, :]
    div = (r / dim).double()
    return torch.cat([torch.sin(div), torch.cos(div)], 1).float()


RankStage = collections.namedtuple('RankStage', 'prob boxes rank_idx sorted_score sorted_bbox class_boxes class_max')


def rank_stage(cls_score, bbox_pred, rois, im_info, first_n, class_agnostic=True, means=None, stds=None, n_valid=None, out=None):
    """The ranking both branches share (learn_nms.py:275-321): softmax + box refinement, then the per-class sort.
    cls_score [B,N,C+1] fp32, bbox_pred [B,N,8] ([B,N,4*(C+1)] class-specific: every foreground class refined from its own columns), rois [B,N,5],
    im_info [B,3]; means / stds: 4 floats or None; n_valid [B] int32: rows past it are padding (probability 0: they sort last).
    out = (prob, boxes) pre-allocated (ops.lnms_prepare).  -> RankStage(prob [B,N,C], boxes [B,N,4] | [B,N,C,4], rank_idx [B,C,F] int32,
    sorted_score [B,F,C], sorted_bbox [B,F,C,4], class_boxes [B,C,F,4], class_max [B,C])."""
    prob, boxes = ops.lnms_prepare(cls_score, bbox_pred, rois, im_info, class_agnostic, means, stds, n_valid, out=out)
    return RankStage(prob, boxes, *ops.lnms_sort(prob, boxes, first_n))


class LearnNMS(object):
    def __init__(self, params, num_fg_classes=80, first_n=100, num_thresh=5, class_thresh=0.01,
                 bbox_means=None, bbox_stds=None, merge_method=-1, score_thresh=1e-3, max_per_image=100,
                 dtype=torch.bfloat16, device='cuda', class_agnostic=True):
        """class_agnostic=False: bbox_pred is [B,N,4*(C+1)] and foreground class k is refined from its own columns 4(k+1)..4(k+1)+3
        (learn_nms.py:283-287); after the per-class sort sorted_bbox[r,k] is class k's box of roi idx[r,k] (:311-321)."""
        t = lambda x, dt: torch.as_tensor(x).to(device=device, dtype=dt).contiguous()
        p = params
        self.dtype, self.device, self.class_agnostic = dtype, device, bool(class_agnostic)
        self.C, self.F, self.T = num_fg_classes, first_n, num_thresh
        self.class_thresh, self.merge, self.score_thresh, self.max_per_image = class_thresh, merge_method, score_thresh, max_per_image
        self.means = None if bbox_means is None else tuple(float(v) for v in bbox_means)
        self.stds = None if bbox_stds is None else tuple(float(v) for v in bbox_stds)
        self.w_emb, self.b_emb = t(p['roi_feat_embedding_weight'], dtype), t(p['roi_feat_embedding_bias'], torch.float32)
        # rank_feat = FC(rank embedding): constant of the weights (learn_nms.py:327-330)
        re = rank_embedding(first_n, 1024).double()
        cpu = lambda x: torch.as_tensor(x).detach().cpu()
        self.rank_feat = t(re @ cpu(p['nms_rank_weight']).double().t() + cpu(p['nms_rank_bias']).double(), torch.float32)
        self.wqk = t(torch.cat([cpu(p['nms_query_1_weight']), cpu(p['nms_key_1_weight'])], 0), dtype)
        self.bqk = t(torch.cat([cpu(p['nms_query_1_bias']), cpu(p['nms_key_1_bias'])], 0), torch.float32)
        # grouped linear_out 16 x (128 -> 8): pad every head's 8 value rows to the 64-wide attention tile
        wo = cpu(p['nms_linear_out_1_weight']).reshape(128, 128).float()
        bo = cpu(p['nms_linear_out_1_bias']).float()
        wpad, bpad = torch.zeros(1024, 128), torch.zeros(1024)
        for h in range(16):
            wpad[h * 64:h * 64 + 8] = wo[h * 8:(h + 1) * 8]
            bpad[h * 64:h * 64 + 8] = bo[h * 8:(h + 1) * 8]
        self.wout_pad, self.bout_pad = t(wpad, dtype), t(bpad, torch.float32)
        pos = SimpleNamespace(wp=cpu(p['nms_pair_pos_fc1_1_weight']).float(), bp=cpu(p['nms_pair_pos_fc1_1_bias']).float())
        self.wp_t, self.bp = pack_pair_pos([pos], device)
        self.w_logit, self.b_logit = t(p['nms_logit_weight'], torch.float32), t(p['nms_logit_bias'], torch.float32)
        self._vwt = {}

    @classmethod
    def from_config(cls, params, cfg, dtype, device):
        """The head of a detector's test graph: no de-normalisation of the deltas (bbox_means / bbox_stds None, symbols/..._learn_nms.py:420-421)."""
        return cls(params, cfg.num_classes - 1, cfg.first_n, len(cfg.nms_target_thresh), cfg.learn_nms_class_thresh, None, None,
                   cfg.merge_method, cfg.score_thresh, cfg.max_per_image, dtype=dtype, device=device, class_agnostic=cfg.class_agnostic)

    def forward(self, cls_score, bbox_pred, rois, im_info, feat, want_detections=True, n_valid=None):
        """cls_score [B,N,C+1] fp32, bbox_pred [B,N,4*num_reg] fp32, rois [B,N,5], im_info [B,3],
        feat = fc_all_2_relu [B,N,1024] -> dict(nms_multi_score [B,F,C,T], sorted_bbox [B,F,C,4],
        sorted_score [B,F,C], nms_final_score [B,F,C], detections ...)."""
        B, N, C1 = cls_score.shape
        C, F = self.C, self.F
        dev = cls_score.device
        # n_valid [B] int32: rows past it are padding (probability 0: they sort last)
        r = rank_stage(cls_score, bbox_pred, rois, im_info, F, self.class_agnostic, self.means, self.stds, n_valid)
        # (feat may carry rows past N -- the gt rows of a training graph: learn_nms.py:335-339 embeds fc_all_2_relu unsliced and
        #  takes rows by rank, so the ranks only ever address its first N rows)
        Nf = feat.shape[1]
        assert Nf >= N
        roi_emb = ops.gemm_nt(feat.reshape(B * Nf, -1).to(self.dtype), self.w_emb, self.b_emb)         # [B*Nf,128]
        x = ops.lnms_embed(roi_emb, self.rank_feat, r.rank_idx)                                        # [B,C,F,128]
        BC = B * C
        xr = x.view(BC, F, 128)
        qk = ops.gemm_nt(xr.reshape(BC * F, 128), self.wqk, self.bqk).view(BC, F, 2048)
        Mpad = ops.pad32(F)
        key = (BC, Mpad, F)            # keyed on F too: pad columns [F, Mpad) must stay zero
        if key not in self._vwt:
            self._vwt[key] = torch.zeros((BC, 1024, Mpad), device=dev, dtype=self.dtype)
        vwt = self._vwt[key]
        ops.gemm_nt(self.wout_pad, xr, out=vwt, n_cols=F)
        bias = ops.geometry_bias(r.class_boxes.view(BC, F, 4), self.wp_t, self.bp, F, half=self.dtype == torch.bfloat16)[0]
        att, _, _ = ops.relation_attention(qk[:, :, :1024], qk[:, :, 1024:], vwt, bias, bout=self.bout_pad, M=F)
        assert self.T == self.w_logit.shape[0]
        multi, final, dets, counts = ops.lnms_score(x, att, self.w_logit, self.b_logit, r.sorted_score, r.sorted_bbox, r.class_max, im_info,
                                                    self.merge, self.class_thresh, self.score_thresh, want_detections)
        out = dict(nms_multi_score=multi, sorted_bbox=r.sorted_bbox, sorted_score=r.sorted_score, nms_final_score=final)
        if want_detections:
            det, det_count, thresh, total = ops.image_topk(dets, counts, self.max_per_image)
            out.update(detections=det, num_detections=det_count, class_dets=dets, class_counts=counts)
        return out


class LearnNMSTrain(object):
    """Train branch of the learn-NMS head (symbols/..._learn_nms.py:424-551) and its adjoint, on a Trainer's parameters.  The trainer owns the
    parameters, their relayout entries and the gradient buffers; this class reaches them as relation.BoxHeadTrain does: w / b / wt, _wg / _bg
    (and _add_wgrad / _add_bgrad for the tensor-operator form), _scratch, the W / Bv gradient views, _relayout.get, deterministic, metrics.

    The element-wise chains of the branch exist in two forms, chosen once per direction by cfg.lnms_fused_glue: single kernels
    (csrc/lnms_train.hip; default) -- `_forward_fused`, `_adjoint_fused` -- and the tensor-operator chains they replaced, kept as the
    reference side of the equality test -- `_forward_chain`, `_adjoint_chain`.  A fused step whose operand its kernel does not take runs
    that step of the chain form."""

    def __init__(self, trainer):
        self.t = trainer

    def __call__(self, cls_score, bbox_pred, rois, im_info, feat, gt_boxes, num_gt, n_valid=None, d_cls_out=None):
        """cls_score [B,N,81] fp32, bbox_pred [B,N,8] ([B,N,4*81] class-specific: learn_nms.py:283-287,311-321) (BlockGrad), rois [B,N,5], feat = fc_all_2_relu[:, :N] bf16.
        Returns (d cls_score [B,N,81] fp32, d feat [B,N,1024] (bf16, as the projection's backward GEMM leaves it), losses); with d_cls_out [B,R,81] fp32 (contiguous, R >= N) the
        class-score gradient is accumulated into d_cls_out[:, :N] instead and None is returned in its place."""
        t, c = self.t, self.t.cfg
        fused = bool(getattr(c, 'lnms_fused_glue', True))
        s = self.forward(cls_score, bbox_pred, rois, im_info, feat, n_valid, self._forward_fused if fused else self._forward_chain)
        B, F, Tn, det = s.B, s.F, s.Tn, t.deterministic
        target = ops.nms_multi_target(s.sorted_bbox, gt_boxes, s.sorted_score, num_gt, c.nms_target_thresh)
        pos, neg, d_multi = losses.nms_loss(s.multi, target, F, Tn, c.nms_loss_scale, c.nms_pos_scale, c.nms_eps)
        lo = dict(nms_pos_loss=T.scalar_sum(pos, 1.0 / B, deterministic=det), nms_neg_loss=T.scalar_sum(neg, 1.0 / B, deterministic=det), nms_multi_score=s.multi, nms_multi_target=target,
                  sorted_score=s.sorted_score, nms_rank_idx=s.rank_idx, nms_class_boxes=s.class_boxes)
        if t.metrics is not None:           # NMSLoss_pos / _neg (B images: one image = one executor in the reference), NMSAcc_pos / _neg
            t.metrics.add_nms(target, s.cond, pos, neg, B)
            lo.update(nms_conditional_score=s.cond, nms_pos_loss_map=pos, nms_neg_loss_map=neg)
        d_cls, d_feat = (self._adjoint_fused if fused else self._adjoint_chain)(s, d_multi, d_cls_out)
        return d_cls, d_feat, lo

    # ---- forward ----------------------------------------------------------------------------------------------
    def forward(self, cls_score, bbox_pred, rois, im_info, feat, n_valid, glue):
        """Rank, embed, then `glue` (module operands, relation module, duplicate classifier) -> the state the adjoint needs."""
        t, c = self.t, self.t.cfg
        B, N, C1 = cls_score.shape
        s = SimpleNamespace(B=B, N=N, C=C1 - 1, F=c.first_n, Tn=len(c.nms_target_thresh), n_valid=n_valid)
        r = rank_stage(cls_score.contiguous(), bbox_pred.contiguous(), rois, im_info, s.F, t.class_agnostic, c.bbox_means, c.bbox_stds, n_valid)
        s.prob, s.boxes, s.rank_idx, s.sorted_score, s.sorted_bbox, s.class_boxes = r.prob, r.boxes, r.rank_idx, r.sorted_score, r.sorted_bbox, r.class_boxes
        rank_feat = ops.gemm_nt(t.rank_emb, t.w('nms_rank'), t.b('nms_rank'), out_dtype=torch.float32)      # [F,128]
        s.feat2 = feat.contiguous().view(B * N, -1)
        roi_emb = ops.gemm_nt(s.feat2, t.w('roi_feat_embedding'), t.b('roi_feat_embedding'))
        s.xr = ops.lnms_embed(roi_emb, rank_feat, s.rank_idx).view(B * s.C, s.F, 128)
        # relation module over (image, class): 16 heads x 64 for Q/K, each head's 8 output channels padded to a 64-wide tile
        s.mod = SimpleNamespace(wqk=t.w('nms_qk_1'), bqk=t.b('nms_qk_1'),
                                wout=t._scratch('nms_wout_pad', (1024, 128), torch.bfloat16),          # persistent: the 56 pad rows of every head stay zero
                                bout=t._scratch('nms_bout_pad', (1024,), torch.float32),
                                wp=t.W.view(t.W.master, 'nms_pair_pos_fc1_1'), bp=t.b('nms_pair_pos_fc1_1'))
        s.cb = s.class_boxes.view(B * s.C, s.F, 4)
        s.lcache = {}
        glue(s)
        return s

    def _attention(self, s, bias):
        """The class-batched relation module on the padded operands -> att [BC,F,1024] (8 real columns per head)."""
        return _module_forward(s.xr, s.mod, bias, s.F, True, False, False, vwt_buf=self.t._scratch('vwt_nms_%d' % s.F, (s.B * s.C, 1024, bias.shape[-1]), torch.bfloat16),
                               cache=s.lcache)[0]

    def _forward_fused(self, s):
        t = self.t
        # the four padded operands of the step (Wout / bout per head, the 64-row logit matrix) refreshed by one launch
        s.w_logit, b_logit = t._scratch('nms_wlogit_pad', (64, 128), torch.bfloat16), t._scratch('nms_blogit_pad', (64,), torch.float32)
        ops.lnms_pad_params(t.w('nms_linear_out_1'), t.b('nms_linear_out_1'), t.w('nms_logit'), t.b('nms_logit'), s.mod.wout, s.mod.bout, s.w_logit, b_logit)
        wp_t, bp = pack_pair_pos([s.mod], s.xr.device)
        if s.n_valid is None and t.class_agnostic:
            # ln G once per IMAGE (B N^2 pairs instead of B C F^2: 9 x fewer at 300 rois / 80 classes / first_n 100), then gathered per class by its ranks
            # (relnet_lnms_gather_bias): the class's boxes are the image's boxes re-ordered, same arithmetic on the same pairs -> bit-identical
            assert s.boxes.shape == (s.B, s.N, 4), "the per-image shortcut needs ONE box per roi (class-agnostic regression)"
            bias = ops.lnms_gather_bias(ops.geometry_bias(s.boxes, wp_t, bp, s.N, fast32=True)[0], s.rank_idx)      # [B,16,N,Npad] -> [BC,16,F,Fpad]
        else:       # (class-specific boxes: a class's boxes are NOT the image's boxes re-ordered, every class has its own N -- the shortcut's premise is false)
            bias = ops.geometry_bias(s.cb, wp_t, bp, s.F, fast32=True)[0]
        s.allf = ops.lnms_residual_relu(self._attention(s, bias), s.xr)                                     # [BC,F,128]
        logit64 = ops.gemm_nt(s.allf.view(-1, 128), s.w_logit, b_logit, out_dtype=torch.float32)            # [BC*F, 64], T real columns
        s.cond, s.multi = ops.lnms_cond_multi(logit64, s.sorted_score, s.Tn)

    def _forward_chain(self, s):
        t, B, C, F, Tn = self.t, s.B, s.C, s.F, s.Tn
        dev = s.xr.device
        s.mod.wout.view(16, 64, 128)[:, :8] = t.w('nms_linear_out_1').view(16, 8, 128)
        s.mod.bout.view(16, 64)[:, :8] = t.b('nms_linear_out_1').view(16, 8)
        wp_t, bp = pack_pair_pos([s.mod], dev)
        bias = ops.geometry_bias(s.cb, wp_t, bp, F, fast32=True)[0]
        att128 = self._attention(s, bias).view(B * C, F, 16, 64)[..., :8].reshape(B * C, F, 128)
        s.allf = torch.relu(s.xr + att128).contiguous()
        s.w_logit = torch.zeros((64, 128), device=dev, dtype=torch.bfloat16); s.w_logit[:Tn] = t.w('nms_logit')
        b_logit = torch.zeros(64, device=dev, dtype=torch.float32); b_logit[:Tn] = t.b('nms_logit')
        logit = ops.gemm_nt(s.allf.view(-1, 128), s.w_logit, b_logit, out_dtype=torch.float32)[:, :Tn]
        s.cond = torch.sigmoid(logit).view(B, C, F, Tn).permute(0, 2, 1, 3).contiguous()                    # [B,F,C,T]
        s.multi = s.sorted_score.unsqueeze(3) * s.cond

    # ---- adjoint ----------------------------------------------------------------------------------------------
    def _adjoint_fused(self, s, d_multi, d_cls_out):
        t, bt = self.t, torch.bfloat16
        BC, F, Tn, det = s.B * s.C, s.F, s.Tn, self.t.deterministic
        d_sorted, d_logit_p = ops.lnms_cond_bwd(d_multi, s.cond, s.sorted_score)
        wl_t = t.wt('nms_logit')
        if wl_t is not None:
            # logit layer backward on the step's own machinery: W^T from the relayout table, the weight gradient in the bucket's grouped launch
            # (Tn real of 64 padded output columns), the bias gradient in its grouped column sum (was 8 library launches: transpose, fills, casts, sums)
            d_allf = ops.gemm_nt(d_logit_p, wl_t)
            T._wg_call(t._wg('nms_logit'), d_logit_p, s.allf.view(BC * F, 128), cout=Tn)
            T.colsum_add(d_logit_p[:, :Tn], *t._bg('nms_logit'))
        else:
            d_allf = self._logit_bwd_chain(s, d_logit_p)
        d_x = self._module_adjoint(s, d_allf)
        if d_x.is_contiguous():
            d_rank = torch.zeros((F, 128), device=d_x.device, dtype=torch.float32)                 # sum over (image, class): one column-sum launch (fp32 accumulation)
            T.colsum_add(d_x.view(BC, F * 128), d_rank.view(-1), deterministic=det)
            T._wg_call(t._wg('nms_rank'), d_rank.to(bt), t.rank_emb)
            T.colsum_add(d_rank, *t._bg('nms_rank'))
        else:
            self._rank_bwd_chain(d_x)
        if d_x.dtype == bt and d_x.is_contiguous() and s.C <= 128:
            d_emb = ops.lnms_take_bwd(d_x, s.rank_idx, s.N)           # every row written: gathered per roi over the classes that rank it (fp32 sums)
        else:
            d_emb = self._take_bwd_chain(s, d_x)
        d_feat, d_prob = self._embed_adjoint(s, d_emb, d_sorted)
        if d_cls_out is not None and d_cls_out.is_contiguous() and d_cls_out.dtype == torch.float32 and d_cls_out.shape[2] == s.C + 1:
            ops.lnms_softmax_bwd(s.prob, d_prob, d_cls_out)
            return None, d_feat
        return self._softmax_bwd_chain(s, d_prob), d_feat

    def _adjoint_chain(self, s, d_multi, d_cls_out):
        BC, F, Tn = s.B * s.C, s.F, s.Tn
        d_sorted = (d_multi * s.cond).sum(3)                                                      # [B,F,C]
        d_logit = (d_multi * s.sorted_score.unsqueeze(3) * s.cond * (1.0 - s.cond)).permute(0, 2, 1, 3).reshape(BC * F, Tn)
        d_logit_p = torch.zeros((BC * F, 64), device=d_logit.device, dtype=torch.bfloat16); d_logit_p[:, :Tn] = d_logit
        d_x = self._module_adjoint(s, self._logit_bwd_chain(s, d_logit_p))
        self._rank_bwd_chain(d_x)
        d_feat, d_prob = self._embed_adjoint(s, self._take_bwd_chain(s, d_x), d_sorted)
        return self._softmax_bwd_chain(s, d_prob), d_feat

    def _logit_bwd_chain(self, s, d_logit_p):
        t = self.t
        d_allf, dw, db = T.linear_bwd(s.allf.view(-1, 128), s.w_logit, d_logit_p, w_t=None, keep_splits=True)
        t._add_wgrad('nms_logit', dw.sum(0)[:s.Tn]); t._add_bgrad('nms_logit', db[:s.Tn])
        return d_allf

    def _module_adjoint(self, s, d_allf):
        """ReLU, residual and relation module backward: d allf [BC*F,128] -> d x [B,C,F,128] (bf16: residual + module); the module's
        parameter gradients go straight into the flat buffers."""
        t, bt = self.t, torch.bfloat16
        BC, F, det = s.B * s.C, s.F, self.t.deterministic
        g = T.relu_bwd(d_allf, s.allf.view(BC * F, 128))                                       # [BC*F,128] bf16
        dY = t._scratch('nms_dy_pad', (BC, F, 1024), bt)                     # persistent: columns 8 .. 63 of every head stay zero
        dY.view(BC, F, 16, 64)[..., :8] = g.view(BC, F, 16, 8)
        # gradients through relation.GradSink: [dQ | dK | dVW] packed once, ONE projection-backward GEMM (K = 3072) with the residual
        # gradient g in its epilogue; the [Wq; Wk] product goes straight into the flat buffer, the padded Wout product through a
        # [1024, 128] scratch whose 8 real rows per head are then added to the compact [128, 128] gradient
        wcat_t = t._relayout.get('rel_cat_nms')
        assert wcat_t is not None
        gq = t.W.view(t.W.grad, 'nms_qk_1')
        glo = t._scratch('nms_dwout_pad', (1024, 128), torch.float32)
        glo.zero_()

        def wg(dy2d, x2d):
            ops.wgrad_tn(dy2d[:, :2048], x2d, out=gq.view(2048, 128), deterministic=det)
            ops.wgrad_tn(dy2d[:, 2048:], x2d, out=glo, deterministic=det)
        sink = GradSink(wcat_t, g.view(BC, F, 128), wg, t._bg('nms_qk_1'), None,
                        t.W.view(t.W.grad, 'nms_pair_pos_fc1_1'), t.Bv.view(t.Bv.grad, 'nms_pair_pos_fc1_1'), t._scratch, deterministic=det)
        r = attention_module_backward(s.xr, s.cb, None, dY, nongt_dim=F, index=1, dtype=bt, packed=s.mod, cache=s.lcache, sink=sink)
        t.W.view(t.W.grad, 'nms_linear_out_1').view(16, 8, 128).add_(glo.view(16, 64, 128)[:, :8])
        T.colsum_add(g.view(BC * F, 128), *t._bg('nms_linear_out_1'))       # (dY's real columns are g's columns)
        return r['d_roi_feat'].view(s.B, s.C, F, 128)

    def _rank_bwd_chain(self, d_x):
        t = self.t
        d_rank = d_x.sum((0, 1), dtype=torch.float32)                                           # [F,128] (fp32 accumulation whatever d_x's dtype)
        t._add_wgrad('nms_rank', T.wgrad(d_rank.to(torch.bfloat16), t.rank_emb)); t._add_bgrad('nms_rank', d_rank.sum(0))

    def _take_bwd_chain(self, s, d_x):
        bt = torch.bfloat16
        if self.t.deterministic and d_x.is_contiguous() and d_x.dtype in (bt, torch.float32):
            # the ordered gather for the operands relnet_lnms_take_bwd does not take (no index_add_: torch's scatter adds with float atomics)
            return ops.lnms_take_bwd_ordered(d_x, s.rank_idx, s.N).to(bt)
        if self.t.deterministic:
            raise ValueError("deterministic training: the learn-NMS take adjoint needs a contiguous bf16 / fp32 gradient (index_add_ uses float atomics)")
        d_emb = torch.zeros((s.B * s.N, 128), device=d_x.device, dtype=torch.float32)
        flat = (s.rank_idx.long() + (torch.arange(s.B, device=d_x.device) * s.N).view(s.B, 1, 1)).view(-1)
        d_emb.index_add_(0, flat, d_x.reshape(-1, 128).float())                                 # take() backward (a roi is ranked in up to 80 classes: fp32 sums)
        return d_emb.to(bt)

    def _embed_adjoint(self, s, d_emb, d_sorted):
        """roi_feat_embedding backward -> d feat [B,N,1024]; sort / slice backward -> d prob [B,N,C]
        (d_prob[b, rank_idx[b,c,f], c] += d_sorted[b,f,c])."""
        t = self.t
        d_feat, dw, db = T.linear_bwd(s.feat2, t.w('roi_feat_embedding'), d_emb, w_t=t.wt('roi_feat_embedding'), keep_splits=True, wgrad_to=t._wg('roi_feat_embedding'), bgrad_to=t._bg('roi_feat_embedding'))
        t._add_bgrad('roi_feat_embedding', db)
        return d_feat.view(s.B, s.N, -1), ops.lnms_scatter_bwd(d_sorted.contiguous(), s.rank_idx, s.N)

    def _softmax_bwd_chain(self, s, d_prob):
        """cls_prob -> softmax backward (the background column has no direct gradient)."""
        p_bg = 1.0 - s.prob.sum(2, keepdim=True)
        inner = (s.prob * d_prob).sum(2, keepdim=True)
        return torch.cat([-p_bg * inner, s.prob * (d_prob - inner)], 2)

