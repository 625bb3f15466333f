"""Box predictors -- MI355X counterparts of
  * SupervisedDetectorOutputsBase      /root/reference/modeling/roi_heads/fast_rcnn.py:293-468
  * SupervisedDetectorOutputsFineTune  /root/reference/modeling/roi_heads/fast_rcnn.py:471-533
  * WeakDetectorOutputsBase            /root/reference/modeling/roi_heads/weak_detector_fast_rcnn.py:39-519 (TYPE "OICR" and "PCL",
                                       with or without REGRESSION_BRANCH)
Parameter names equal the reference's (`cls_score_delta`, `bbox_pred_delta`, `cls_score_ft`, `bbox_pred_ft`,
`weak_detector_head.{classifier_stream,detection_stream,oicr_predictors.k,regression_branch_cls,regression_branch_bbox}`, `embeddings.weight`).
All Linear layers that share an input run as one fused GEMM (LinearGroup); the loss kernels emit loss + gradient."""
import os

import torch
from torch import nn

from .. import ops
from ..layers import Linear, LinearGroup
from ..structures import FAST_RCNN_REGISTRY, WEAK_DETECTOR_FAST_RCNN_REGISTRY


REGRESSION_LOSSES = ["loss_regression_cls", "loss_regression_bbox"]          # FastRCNNOutputsRegression.losses weak_detector_fast_rcnn.py:35-36


def _box_loss_cfg(cfg):
    """(BBOX_REG_LOSS_TYPE, SMOOTH_L1_BETA) of fast_rcnn.py:70-87, checked"""
    bh = cfg.MODEL.ROI_BOX_HEAD
    loss_type, beta = str(bh.BBOX_REG_LOSS_TYPE), float(bh.SMOOTH_L1_BETA)
    if loss_type not in ops.BOX_LOSS_TYPES:
        raise ValueError(f"Invalid bbox reg loss type '{loss_type}'")
    if not beta >= 0.0:
        raise ValueError(f"MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA must be >= 0, got {beta}")
    return loss_type, beta


def _detect(head, probs, bbox, proposals):
    """d2 fast_rcnn_inference (drop bg, apply_deltas, clip, score > thresh, per-class NMS, top-k) on the device, for ragged
    probabilities [R, K + 1] / deltas [R, 4K] -> (list[Instances(pred_boxes, scores, pred_classes)], list[filter_inds])"""
    from .inference import pack_proposal_instances
    from ..structures import Boxes, Instances
    dev, k = probs.device, head.num_classes
    props, pcount = pack_proposal_instances(proposals, dev)
    n, rcap = props.shape[0], props.shape[1]
    pp = torch.zeros((n * rcap, k + 1), dtype=torch.float32, device=dev)
    bb = torch.zeros((n * rcap, 4 * k), dtype=torch.float32, device=dev)
    o = 0
    for i, p in enumerate(proposals):      # ragged -> fixed slots (API boundary; the fused eval path never leaves fixed slots)
        pp[i * rcap:i * rcap + len(p)], bb[i * rcap:i * rcap + len(p)] = probs[o:o + len(p)], bbox[o:o + len(p)].float()
        o += len(p)
    hw = torch.tensor([p.image_size for p in proposals], dtype=torch.float32).to(dev)
    boxes, sc, cls, roi, cnt = ops.detections(pp, bb, props, pcount, hw, head.bbox_reg_weights, head.test_score_thresh,
                                              head.test_nms_thresh, head.test_topk_per_image)
    res, inds = [], []
    for i, c in enumerate(cnt.tolist()):
        res.append(Instances(proposals[i].image_size, pred_boxes=Boxes(boxes[i, :c]), scores=sc[i, :c], pred_classes=cls[i, :c].long()))
        inds.append(roi[i, :c].long())
    return res, inds


def _freeze_by_first_component(module, layers):
    for name, p in module.named_parameters():
        if any(layer == name.split(".")[0] for layer in layers):
            p.requires_grad = False


@WEAK_DETECTOR_FAST_RCNN_REGISTRY.register()
class WeakDetectorOutputsBase(nn.Module):
    def __init__(self, cfg, input_shape):
        super().__init__()
        wd = cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR
        assert wd.TYPE in ("OICR", "PCL"), "WEAK_DETECTOR.TYPE is \"OICR\" or \"PCL\""
        assert not wd.OICR_REGRESSION_BRANCH, \
            ("WEAK_DETECTOR.OICR_REGRESSION_BRANCH (a box regressor per refinement stream) is not supported: the reference's own non-TTA inference "
             "hands the list of per-stream deltas to apply_deltas (weak_detector_fast_rcnn.py:176-179, 270-277). REGRESSION_BRANCH is supported")
        self.regression_branch = bool(wd.REGRESSION_BRANCH)
        assert not self.regression_branch or wd.OICR_ITER > 0, \
            "WEAK_DETECTOR.REGRESSION_BRANCH needs OICR_ITER > 0: its pseudo-GT comes from the mean of the refinement streams (:248)"
        assert wd.TYPE != "PCL" or wd.NUM_KMEANS_CLUSTER == 3, \
            "TYPE \"PCL\" needs NUM_KMEANS_CLUSTER == 3: the only k-means the device kernel restates (csrc/pcl.hip, tests/golden/pcl_kmeans.py)"
        self.weak_detector_type = wd.TYPE
        self.graph_iou_threshold, self.max_pc_num = wd.GRAPH_IOU_THRESHOLD, wd.MAX_PC_NUM
        self.num_classes = cfg.MODEL.ROI_HEADS.NUM_CLASSES
        self.oicr_iter = wd.OICR_ITER
        self.fg_threshold, self.bg_threshold = wd.FG_THRESHOLD, wd.BG_THRESHOLD
        self.mil_multiplier = wd.MIL_MULTIPLIER
        self.detector_temp, self.classifier_temp = wd.DETECTOR_TEMP, wd.CLASSIFIER_TEMP
        self.input_size = input_shape.channels * (input_shape.width or 1) * (input_shape.height or 1)
        k = self.num_classes
        self.classifier_stream = Linear(self.input_size, k)
        self.detection_stream = Linear(self.input_size, k)
        nn.init.normal_(self.classifier_stream.weight, std=0.01)
        nn.init.normal_(self.detection_stream.weight, std=0.01)
        self.oicr_predictors = nn.ModuleList([Linear(self.input_size, k + 1) for _ in range(self.oicr_iter)])
        for l in self.oicr_predictors:
            nn.init.normal_(l.weight, std=0.01)
        members = [self.classifier_stream, self.detection_stream] + list(self.oicr_predictors)
        if self.regression_branch:          # :93-99 -- two more column blocks of the head's one fused GEMM / weight-gradient launch
            self.regression_branch_cls = Linear(self.input_size, k + 1)
            self.regression_branch_bbox = Linear(self.input_size, 4 * k)
            nn.init.normal_(self.regression_branch_bbox.weight, std=0.001)
            nn.init.normal_(self.regression_branch_cls.weight, std=0.01)
            members += [self.regression_branch_cls, self.regression_branch_bbox]
            self.box_reg_loss_type, self.smooth_l1_beta = _box_loss_cfg(cfg)
        self.bbox_reg_weights = tuple(cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS)
        self.test_score_thresh = cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST
        self.test_nms_thresh = cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST
        self.test_topk_per_image = cfg.TEST.DETECTIONS_PER_IMAGE
        _freeze_by_first_component(self, cfg.MODEL.FREEZE_LAYERS.FAST_RCNN)
        self.group = LinearGroup(members)
        self.col_cls, self.col_det = self.group.cols[0], self.group.cols[1]
        self.col_oicr = self.group.cols[2:2 + self.oicr_iter]
        if self.regression_branch:
            self.col_reg_cls, self.col_reg_bbox = self.group.cols[2 + self.oicr_iter:]
            assert all(b - a == k + 1 for a, b in zip(self.col_oicr, self.col_oicr[1:]))          # unit_softmax_mean: equally spaced streams

    @property
    def n_losses(self):
        """loss_im_cls, loss_oicr_1..n (+ loss_regression_cls, loss_regression_bbox)"""
        return 1 + self.oicr_iter + (2 if self.regression_branch else 0)

    # ---- what the supervised predictor adds to its own outputs (fast_rcnn.py:360-374): the columns of this head's fused Linear that carry
    # the weak scores -- the refinement streams, whose mean is taken, or regression_branch_cls alone (:363-364)
    @property
    def score_cols(self):
        return (self.col_reg_cls, 1) if self.regression_branch else (self.col_oicr[0], self.oicr_iter)

    def prepare(self, dtype, version):
        self.group.prepare(dtype, version)

    # ---- a12: WeakDetectorOutputsBase.losses weak_detector_fast_rcnn.py:189-255 (fused fwd + gradient into `dy`)
    def fused_losses(self, lin, rois5, valid, rois_per_image, n_images, multihot, loss_out, grad_dtype, side_stream=None, reg_loss_out=None):
        """lin fp32 [Rw, kp] = fused Linear outputs on the weak RoIs. Returns dy [Rw, kp] (grad_dtype).
        REGRESSION_BRANCH (:245-254): reg_loss_out [2] receives loss_regression_cls / loss_regression_bbox; the branch's four launches
        (mean score, pseudo-GT with boxes, weighted cross-entropy, box loss) read forward outputs only, so they go where iterations >= 1 go.
        Only OICR iteration 0 needs the MIL output x_r; iterations >= 1 take their pseudo-GT from softmax(oicr_{k-1} logits),
        which are forward outputs: with `side_stream` they run beside the (single-workgroup-per-image, latency-bound) MIL
        kernel instead of behind it. Every launch writes its own columns of dy / its own loss slot."""
        k = self.num_classes
        dy = ops.zeros((lin.shape[0], self.group.kp), grad_dtype, lin.device)
        # more than 1024 rows per image (MODEL.LOAD_PROPOSALS): the targets kernel's wide form; at or below, the launch it always was
        wide = dict(wide=True) if rois_per_image > 1024 else {}

        def oicr(it, xr):
            if it == 0:
                lab, wts = ops.oicr_targets(xr, 0, 0, k, rois5, valid, rois_per_image, n_images, multihot, self.fg_threshold, self.bg_threshold,
                                            **wide)
            else:
                lab, wts = ops.oicr_targets(lin, self.col_oicr[it - 1], 1, k, rois5, valid, rois_per_image, n_images, multihot,
                                            self.fg_threshold, self.bg_threshold, **wide)
            ops.softmax_ce(lin, self.col_oicr[it], k + 1, lab, weights=wts, dy=dy, dcol0=self.col_oicr[it], loss_out=loss_out[1 + it:2 + it])

        def regression():
            """:245-254: pseudo-GT from the mean of the refinement streams' softmaxes, FastRCNNOutputsRegression on the branch's two outputs"""
            step = self.col_oicr[1] - self.col_oicr[0] if self.oicr_iter > 1 else 0
            mean = ops.softmax_mean(lin, self.col_oicr[0], step, self.oicr_iter, k, valid)
            if self.weak_detector_type == "PCL":          # :252 -- the "next iteration" is regression_branch_cls; its pc_* tables are not consumed
                t = ops.pcl_targets(mean, 0, 0, lin, self.col_reg_cls, 1, k, rois5, valid, rois_per_image, n_images, multihot,
                                    ldc=self.max_pc_num * k, fg_thresh=self.fg_threshold, bg_thresh=self.bg_threshold,
                                    graph_iou_thresh=self.graph_iou_threshold, max_pc_num=self.max_pc_num, want_boxes=True)
                lab, wts, gtb = t["labels"][0], t["cls_weights"][0], t["gt_boxes"][0]
            else:
                lab, wts, gtb = ops.oicr_targets(mean, 0, 0, k, rois5, valid, rois_per_image, n_images, multihot, self.fg_threshold,
                                                 self.bg_threshold, want_boxes=True, **wide)
            ops.softmax_ce(lin, self.col_reg_cls, k + 1, lab, weights=wts, dy=dy, dcol0=self.col_reg_cls, loss_out=reg_loss_out[0:1])
            ops.box_reg_loss(lin, self.col_reg_bbox, k, lab, rois5, gtb, self.bbox_reg_weights, dy=dy, dcol0=self.col_reg_bbox,
                             loss_out=reg_loss_out[1:2], loss_type=self.box_reg_loss_type, beta=self.smooth_l1_beta)

        reg = self.regression_branch
        assert not reg or reg_loss_out is not None, "REGRESSION_BRANCH: fused_losses needs reg_loss_out [2]"

        def pcl(its, xr):
            """TYPE "PCL" (:225-238): unit_pcl_targets for the consecutive iterations `its` in one launch, then unit_pcl_loss per stream.
            PCLFunction.backward ignores grad_output, so the reference's refinement gradient carries neither the 1 / images of the
            loss's mean nor any loss weight: gscale is 1 whatever the image count."""
            cols = self.col_oicr
            step = cols[1] - cols[0] if self.oicr_iter > 1 else 0
            if any(cols[i + 1] - cols[i] != step for i in range(self.oicr_iter - 1)):       # (never with equal-width predictors)
                for it in its[1:]:
                    pcl([it], xr)
                its = its[:1]
            first = its[0]
            src, col0, mode = (xr, 0, 0) if first == 0 else (lin, cols[first - 1], 1)
            assert first > 0 or len(its) == 1
            t = ops.pcl_targets(src, col0, mode, lin, cols[first], 1, k, rois5, valid, rois_per_image, n_images, multihot,
                                ldc=self.max_pc_num * k, n_streams=len(its), step=step, nstep=step, fg_thresh=self.fg_threshold,
                                bg_thresh=self.bg_threshold, graph_iou_thresh=self.graph_iou_threshold, max_pc_num=self.max_pc_num)
            for j, it in enumerate(its):
                ops.pcl_loss(lin, cols[it], k, valid, rois_per_image, n_images, t["labels"][j], t["cls_weights"][j], t["gt_assign"][j],
                             t["pc_count"][j], t["pc_img_cls_weights"][j], t["pc_probs"][j], t["n_pc"][j], dy=dy, dcol0=cols[it], gscale=1.0,
                             loss_out=loss_out[1 + it:2 + it])

        if self.weak_detector_type == "PCL":
            later = list(range(1, self.oicr_iter))
            if side_stream is not None and (later or reg):
                side_stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side_stream):
                    if later:
                        pcl(later, None)
                    if reg:
                        regression()
            _, xr = ops.wsddn_mil(lin, self.col_cls, self.col_det, k, valid, rois_per_image, n_images, multihot, self.classifier_temp,
                                  self.detector_temp, self.mil_multiplier, dy=dy, dyc0=self.col_cls, dyd0=self.col_det, loss_out=loss_out[0:1])
            if self.oicr_iter > 0:
                pcl([0], xr)
            if side_stream is not None and (later or reg):
                torch.cuda.current_stream().wait_stream(side_stream)
            else:
                if later:
                    pcl(later, None)
                if reg:
                    regression()
            return dy

        on_side = side_stream is not None and (self.oicr_iter > 1 or reg)
        if on_side:
            main = torch.cuda.current_stream()
            side_stream.wait_stream(main)                    # dy zeroed, lin complete
            with torch.cuda.stream(side_stream):
                for it in range(1, self.oicr_iter):
                    oicr(it, None)
                if reg:
                    regression()
        _, xr = ops.wsddn_mil(lin, self.col_cls, self.col_det, k, valid, rois_per_image, n_images, multihot, self.classifier_temp,
                              self.detector_temp, self.mil_multiplier, dy=dy, dyc0=self.col_cls, dyd0=self.col_det, loss_out=loss_out[0:1])
        oicr(0, xr)
        if on_side:
            torch.cuda.current_stream().wait_stream(side_stream)
        else:
            for it in range(1, self.oicr_iter):
                oicr(it, None)
            if reg:
                regression()
        return dy


    # ---- plugin surface: the reference's signatures (weak_detector_fast_rcnn.py:148,167,189,270-306). Forward values only: the
    # training gradient path is the fused step (fused_losses above), these are for evaluation / monitoring / module-level tests.
    def _lin(self, x_weak):
        dtype = getattr(self, "compute_dtype", torch.bfloat16)
        self.prepare(dtype, getattr(self, "_version", 0))
        return self.group.fwd(ops.cast(x_weak.contiguous(), dtype))

    def forward(self, x_weak):
        """:148-165 -> ([classifier_stream / T_cls, detection_stream / T_det, [oicr_k], [], regression_cls, regression_bbox], None) in training
        (the last two None without REGRESSION_BRANCH; the outputs carry an autograd graph: one node over the fused Linear,
        modeling/train_modules.py), `evaluation(x_weak)` otherwise"""
        if not self.training:
            return self.evaluation(x_weak)
        from .train_modules import _WeakPredictFn, _anchor
        k = self.num_classes
        x = x_weak if x_weak.requires_grad else x_weak + _anchor(self, x_weak.device) * 0          # (the node's parameters are updated by its explicit backward)
        lin = _WeakPredictFn.apply(x, self)
        cs = lin[:, self.col_cls:self.col_cls + k] / self.classifier_temp
        ds = lin[:, self.col_det:self.col_det + k] / self.detector_temp
        rc = lin[:, self.col_reg_cls:self.col_reg_cls + k + 1] if self.regression_branch else None
        rb = lin[:, self.col_reg_bbox:self.col_reg_bbox + 4 * k] if self.regression_branch else None
        return [cs, ds, [lin[:, c:c + k + 1] for c in self.col_oicr], [], rc, rb], None

    @torch.no_grad()
    def evaluation(self, x_weak):
        """:167-187 -> ([regression_cls, regression_bbox], None) under REGRESSION_BRANCH (:169-171); otherwise (OICR_ITER > 0)
        ([[oicr_k logits], zeros(R, 4K)], None)"""
        lin, k = self._lin(x_weak), self.num_classes
        if self.regression_branch:
            return [lin[:, self.col_reg_cls:self.col_reg_cls + k + 1], lin[:, self.col_reg_bbox:self.col_reg_bbox + 4 * k]], None
        return [[lin[:, c:c + k + 1] for c in self.col_oicr], torch.zeros((lin.shape[0], 4 * k), device=lin.device)], None

    def losses(self, weak_predictions, weak_proposals, weak_targets):
        """:189-255 -> {'loss_im_cls', 'loss_oicr_1..n'} (+ {'loss_regression_cls', 'loss_regression_bbox'} under REGRESSION_BRANCH) (HIP kernels unit_wsddn_mil / unit_oicr_targets / unit_softmax_ce; TYPE "PCL":
        unit_pcl_targets / unit_pcl_loss, whose refinement gradient ignores the weight that arrives, as PCLFunction.backward does). With predictions
        that carry a graph (training-mode forward) the losses do too: one autograd node whose backward hands out the gradient the loss kernels
        emit, scaled by the weight that arrives. weak_predictions = forward()'s list, weak_proposals = list[Instances(proposal_boxes)],
        weak_targets = list[LongTensor]."""
        cs, ds, oicr = weak_predictions[0], weak_predictions[1], weak_predictions[2]
        reg = [weak_predictions[4], weak_predictions[5]] if self.regression_branch else []
        with_graph = torch.is_grad_enabled() and any(t.requires_grad for t in [cs, ds] + list(oicr) + reg)
        with torch.set_grad_enabled(with_graph):
            return self._losses(cs, ds, oicr, weak_proposals, weak_targets, with_graph, reg)

    def _losses(self, cs, ds, oicr, weak_proposals, weak_targets, with_graph, reg=()):
        k, dev = self.num_classes, cs.device
        sizes = [len(p) for p in weak_proposals]
        b, s = len(sizes), max(sizes)
        kp = self.group.kp
        lin = torch.zeros((b * s, kp), dtype=torch.float32, device=dev)
        rois5 = torch.zeros((b * s, 5), dtype=torch.float32, device=dev)
        valid = torch.full((b * s,), -1, dtype=torch.int32, device=dev)
        multihot = torch.zeros((b, k), dtype=torch.uint8, device=dev)
        o = 0
        for i, (n, pr) in enumerate(zip(sizes, weak_proposals)):
            rows = slice(i * s, i * s + n)
            lin[rows, self.col_cls:self.col_cls + k] = cs[o:o + n].float() * self.classifier_temp
            lin[rows, self.col_det:self.col_det + k] = ds[o:o + n].float() * self.detector_temp
            for c, lg in zip(self.col_oicr, oicr):
                lin[rows, c:c + k + 1] = lg[o:o + n].float()
            if self.regression_branch:
                lin[rows, self.col_reg_cls:self.col_reg_cls + k + 1] = reg[0][o:o + n].float()
                lin[rows, self.col_reg_bbox:self.col_reg_bbox + 4 * k] = reg[1][o:o + n].float()
            rois5[rows, 0] = i
            rois5[rows, 1:] = (pr.proposal_boxes.tensor if hasattr(pr.proposal_boxes, "tensor") else pr.proposal_boxes).to(dev)
            valid[rows] = 0
            multihot[i, weak_targets[i].long().to(dev)] = 1
            o += n
        if with_graph:
            from .train_modules import _WeakLossFn
            loss = _WeakLossFn.apply(lin, self, dict(rois5=rois5, valid=valid, s=s, b=b, multihot=multihot))
        else:
            loss = torch.zeros(self.n_losses, dtype=torch.float32, device=dev)
            reg_kw = dict(reg_loss_out=loss[1 + self.oicr_iter:]) if self.regression_branch else {}
            self.fused_losses(lin, rois5, valid, s, b, multihot, loss, torch.float32, **reg_kw)
        out = {"loss_im_cls": loss[0]}
        out.update({f"loss_oicr_{i + 1}": loss[1 + i] for i in range(self.oicr_iter)})
        if self.regression_branch:
            out.update({n: loss[1 + self.oicr_iter + i] for i, n in enumerate(REGRESSION_LOSSES)})
        return out

    def predict_probs(self, predictions, proposals):
        """:280-287: sum_k softmax(oicr_k), or softmax(regression_cls) under REGRESSION_BRANCH (:284-285), split per image"""
        scores, _ = predictions
        if self.regression_branch:
            p = ops.softmax_rows(scores.contiguous().float(), self.num_classes + 1)
        else:
            p = sum(ops.softmax_rows(sc.contiguous().float(), self.num_classes + 1) for sc in scores)
        return p.split([len(q) for q in proposals], dim=0)

    @torch.no_grad()
    def predict_boxes(self, predictions, proposals):
        """:270-278: Box2BoxTransform.apply_deltas of the [R, 4K] deltas on the proposals, split per image (unit_box_decode)"""
        _, deltas = predictions
        tb = lambda v: (v.tensor if hasattr(v, "tensor") else v)
        boxes = torch.cat([tb(p.proposal_boxes) for p in proposals]).to(deltas.device).float().contiguous()
        out = ops.box_decode(deltas.float().contiguous(), boxes, self.bbox_reg_weights, self.num_classes)
        return out.split([len(p) for p in proposals], dim=0)

    @torch.no_grad()
    def inference(self, predictions, proposals, tta=False):
        """:289-306 -> (list[Instances(pred_boxes, scores, pred_classes)], list[filter_inds]) through the detection kernels"""
        if tta:
            raise NotImplementedError("TTA is outside the hot path (SURVEY.md section 2)")
        probs = torch.cat(self.predict_probs(predictions, proposals), 0)
        return _detect(self, probs, predictions[1], proposals)


@FAST_RCNN_REGISTRY.register()
class SupervisedDetectorOutputsBase(nn.Module):
    finetune = False

    def __init__(self, cfg, input_shape):
        super().__init__()
        self.num_classes = k = cfg.MODEL.ROI_HEADS.NUM_CLASSES
        self.box_dim = 4
        bh = cfg.MODEL.ROI_BOX_HEAD
        assert not bh.CLS_AGNOSTIC_BBOX_REG, ("CLS_AGNOSTIC_BBOX_REG: the reference's own similarity transfer reshapes the box deltas to "
                                              "[R, K, 4] (fast_rcnn.py:414), so it cannot run class-agnostic either")
        # fast_rcnn.py:70-87 through :438-445: the box term, "smooth_l1" (with SMOOTH_L1_BETA) or "giou" -- a switch of the loss kernel
        # (unit_box_reg_loss_ex)
        self.box_reg_loss_type, self.smooth_l1_beta = _box_loss_cfg(cfg)
        self.bbox_reg_weights = tuple(cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS)
        self.test_score_thresh = cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST
        self.test_nms_thresh = cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST
        self.test_topk_per_image = cfg.TEST.DETECTIONS_PER_IMAGE
        self.input_size = input_shape.channels * (input_shape.width or 1) * (input_shape.height or 1)
        self.weak_detector_head = WEAK_DETECTOR_FAST_RCNN_REGISTRY.get(cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.NAME)(cfg, input_shape)
        self.cls_score_delta = Linear(self.input_size, k + 1)
        self.bbox_pred_delta = Linear(self.input_size, k * 4)
        self.regression_branch = self.weak_detector_head.regression_branch
        nn.init.constant_(self.cls_score_delta.weight, 0.)       # fast_rcnn.py:319
        if self.regression_branch:
            nn.init.constant_(self.bbox_pred_delta.weight, 0.)   # :322-323: the weak branch's deltas are the starting point
        else:
            nn.init.normal_(self.bbox_pred_delta.weight, std=0.001)  # :321
        emb = None
        path = cfg.MODEL.ROI_HEADS.EMBEDDING_PATH
        if path and os.path.exists(path):
            emb = torch.load(path)["embeddings"].float()         # fast_rcnn.py:327
        if emb is None:
            emb = torch.zeros(80, 300)
        self.embeddings = nn.Embedding.from_pretrained(emb, freeze=True)
        if self.finetune:
            self.cls_score_ft = Linear(self.input_size, k + 1)
            self.bbox_pred_ft = Linear(self.input_size, k * 4)
            for l in (self.cls_score_ft, self.bbox_pred_ft):
                nn.init.constant_(l.weight, 0.)
            self.group_ft = LinearGroup([self.cls_score_ft, self.bbox_pred_ft])
        _freeze_by_first_component(self, cfg.MODEL.FREEZE_LAYERS.FAST_RCNN)
        self.group = LinearGroup([self.cls_score_delta, self.bbox_pred_delta])
        self.col_cls, self.col_bbox = self.group.cols
        self.register_buffer("_novel_mask", torch.zeros(k, dtype=torch.uint8), persistent=False)
        self._novel_mask[list(cfg.DATASETS.FEWSHOT.NOVEL_CLASSES_ID)] = 1

    def prepare(self, dtype, version):
        self.group.prepare(dtype, version)
        self.weak_detector_head.prepare(dtype, version)
        if self.finetune:
            self.group_ft.prepare(dtype, version)

    def get_similarity(self, base_classes, novel_classes, indexer):
        """fast_rcnn.py:376-382 (tiny 5x300 @ 300x15 product: plumbing-size, evaluated once per call)."""
        e = self.embeddings.weight[indexer]
        return torch.mm(e.index_select(0, novel_classes), e.index_select(0, base_classes).transpose(0, 1))

    # ---- a10 + a11: forward (fast_rcnn.py:384-433) + FastRCNNOutputs.losses (:438-445), fused with the gradient
    def sup_losses(self, lin_sup, lin_sup_weak, roi_cls, rois5, roi_gt, loss_out, grad_dtype):
        """lin_sup fp32 [R,kp] = [cls_score_delta | bbox_pred_delta](box_head feat); lin_sup_weak = weak head's fused Linear
        on the (no-grad) weak_box_head features of the same RoIs (None when MULTI_BOX_HEAD is off: box_head feat itself).
        Returns dy [R, kp] in grad_dtype."""
        k = self.num_classes
        wh = self.weak_detector_head
        wcol, wn = wh.score_cols
        scores = ops.sup_scores(lin_sup, self.col_cls, lin_sup_weak, wcol, wn, k + 1, self._novel_mask)
        dy = ops.zeros((lin_sup.shape[0], self.group.kp), grad_dtype, lin_sup.device)
        ops.softmax_ce(scores, 0, k + 1, roi_cls, dy=dy, dcol0=self.col_cls, loss_out=loss_out[0:1])
        bbox, bcol = self.add_weak_deltas(lin_sup, self.col_bbox, lin_sup_weak), (0 if self.regression_branch else self.col_bbox)
        ops.box_reg_loss(bbox, bcol, k, roi_cls, rois5, roi_gt, self.bbox_reg_weights, dy=dy, dcol0=self.col_bbox,
                         loss_out=loss_out[1:2], loss_type=self.box_reg_loss_type, beta=self.smooth_l1_beta)
        return dy, scores

    def add_weak_deltas(self, bbox, col0, lin_weak):
        """fast_rcnn.py:370-374, 426: bbox[:, col0 : col0 + 4K] + regression_branch_bbox(x_weak) as an fp32 [R, 4K] buffer, `bbox` itself
        without the branch. The weak head is evaluated under no_grad there (:388-392), so d(loss)/d(sum) is d(loss)/d(bbox_pred_delta):
        the loss kernel writes it into the bbox_pred_delta columns of dy and nothing else changes. The add is unit_sup_scores, whose
        `delta + mean of ONE block of weak columns` over 4K columns is exactly this sum (s / 1.0f is s): no new kernel, no ATen launch."""
        if not self.regression_branch:
            return bbox
        return ops.sup_scores(bbox, col0, lin_weak, self.weak_detector_head.col_reg_bbox, 1, 4 * self.num_classes)

    @property
    def weak_bbox_col(self):
        """FineTune with REGRESSION_BRANCH: the column of the weak head's box deltas that unit_transfer_predictions_ex adds in its one launch,
        (o + weak) + ft as fast_rcnn.py:526, 528 sums them. None everywhere else: Base with the switch keeps unit_transfer_predictions followed
        by add_weak_deltas, and no other configuration has weak deltas."""
        return self.weak_detector_head.col_reg_bbox if (self.finetune and self.regression_branch) else None

    def transfer(self, lin_sup, lin_weak, sim_cls, sim_bbox, t, ft=None):
        """fast_rcnn.py:401-426 (Base, eval) / :504-528 (FineTune) -> (scores [R, K+1], bbox [R, 4K]) from the Linear outputs: the base -> novel
        transfer, the weak head's scores (and, under REGRESSION_BRANCH, its box deltas) and the ft heads, in the reference's order of additions."""
        wb = self.weak_bbox_col
        scores, bbox = ops.transfer_predictions(lin_sup, self.col_cls, self.col_bbox, self.num_classes, lin_weak, *self.weak_detector_head.score_cols,
                                                sim_cls, sim_bbox, t["base"], t["novel"], t["role"], t["slot"], ft=ft, fccol0=self.col_cls,
                                                fbcol0=self.col_bbox, wbcol0=wb)
        if wb is None:
            bbox = self.add_weak_deltas(bbox, 0, lin_weak)          # Base: after the base -> novel transfer of the supervised deltas (:414-426)
        return scores, bbox


    # ---- plugin surface: the reference's signatures (fast_rcnn.py:384,435,455). Forward values only (see WeakDetectorOutputsBase).
    def _roles(self, novel_classes, base_classes, dev):
        key = (tuple(int(c) for c in novel_classes), tuple(int(c) for c in base_classes), dev)
        if getattr(self, "_roles_key", None) != key:
            k = self.num_classes
            role, slot = torch.zeros(k, dtype=torch.int8), torch.zeros(k, dtype=torch.int32)
            for i, c in enumerate(key[1]):
                role[c], slot[c] = 1, i
            for i, c in enumerate(key[0]):
                role[c], slot[c] = 2, i
            mask = torch.zeros(k, dtype=torch.uint8)
            mask[list(key[0])] = 1
            self._roles_t = dict(base=torch.tensor(key[1], dtype=torch.int32, device=dev), novel=torch.tensor(key[0], dtype=torch.int32, device=dev),
                                 role=role.to(dev), slot=slot.to(dev), novel_mask=mask.to(dev))
            self._roles_key = key
        return self._roles_t

    def forward(self, x, novel_classes, base_classes, supervised_branch_x_weak=None, x_weak=None, similarity=None):
        """fast_rcnn.py:384-433 (Base) / :484-533 (FineTune) -> ([scores [R,K+1], bbox [R,4K]], weak_branch_return). In TRAINING mode with
        autograd enabled the predictions carry a graph (one node over the predictor's explicit forward / backward, train_modules._SupPredictFn);
        otherwise values from the same kernels."""
        if self.training and torch.is_grad_enabled() and x is not None:
            from .train_modules import _SupPredictFn, _anchor
            t = self._roles(novel_classes, base_classes, x.device)
            sim = similarity if self.finetune else None
            xg = x if x.requires_grad else x + _anchor(self, x.device) * 0
            scores, bbox = _SupPredictFn.apply(xg, sim["cls"] if sim is not None else None, sim["bbox"] if sim is not None else None, self,
                                               dict(roles=t, x_sup_weak=supervised_branch_x_weak))
            weak_ret = None
            if x_weak is not None:
                weak_ret, _ = self.weak_detector_head(x_weak)
            return [scores, bbox], weak_ret
        with torch.no_grad():
            return self._forward_values(x, novel_classes, base_classes, supervised_branch_x_weak, x_weak, similarity)

    def _forward_values(self, x, novel_classes, base_classes, supervised_branch_x_weak=None, x_weak=None, similarity=None):
        """the forward of fast_rcnn.py:384-433 / :484-533 as values (eval; training under no_grad)
        x: box-head features [R, D]; supervised_branch_x_weak: weak_box_head features of the same RoIs (None: x itself, :389-390);
        similarity: {'cls': [R,n,b] | [n,b], 'bbox': ...} -- applied in eval (Base) / always (FineTune); training (Base) fills the
        novel columns with -inf (:427-428)."""
        if x is None:
            raise NotImplementedError("x=None (train_only_weak) is outside the hot path (rcnn.py:433 default False)")
        dtype = getattr(self, "compute_dtype", torch.bfloat16)
        self.prepare(dtype, getattr(self, "_version", 0))
        wh, k, dev = self.weak_detector_head, self.num_classes, x.device
        t = self._roles(novel_classes, base_classes, dev)
        xc = ops.cast(x.contiguous(), dtype)
        lin_sup = self.group.fwd(xc)
        lin_w = wh.group.fwd(xc if supervised_branch_x_weak is None else ops.cast(supervised_branch_x_weak.contiguous(), dtype))
        transfer = similarity is not None and (self.finetune or not self.training)
        if transfer or self.finetune:
            r = x.shape[0]
            sims = []
            for h in ("cls", "bbox"):
                sm = similarity[h] if transfer else None
                if sm is not None and sm.dim() == 2:
                    sm = sm[None].expand(r, -1, -1)
                sims.append(sm.float().contiguous() if sm is not None else None)
            ft = self.group_ft.fwd(xc) if self.finetune else None
            scores, bbox = self.transfer(lin_sup, lin_w, sims[0], sims[1], t, ft=ft)
        else:
            wcol, wn = wh.score_cols
            scores = ops.sup_scores(lin_sup, self.col_cls, lin_w, wcol, wn, k + 1, t["novel_mask"] if self.training else None)
            bbox = self.add_weak_deltas(lin_sup, self.col_bbox, lin_w) if self.regression_branch else lin_sup[:, self.col_bbox:self.col_bbox + 4 * k]
        weak_ret = None
        if x_weak is not None:
            weak_ret, _ = wh(x_weak)
        return [scores, bbox], weak_ret

    def losses(self, predictions, proposals, weak_predictions=None, weak_proposals=None, weak_targets=None, train_only_weak=False):
        """fast_rcnn.py:435-453 -> {'loss_cls', 'loss_box_reg'} (+ the weak head's losses); proposals = list[Instances] with
        proposal_boxes, gt_boxes, gt_classes (label_and_sample_proposals' output). HIP kernels unit_softmax_ce / unit_box_reg_loss; with
        predictions that carry a graph (training-mode forward) the losses do too (train_modules._SupLossFn), and may enter the total with
        any weight."""
        out = {}
        if not train_only_weak:
            scores, bbox = predictions
            dev, k = scores.device, self.num_classes
            tb = lambda v: (v.tensor if hasattr(v, "tensor") else v)
            with torch.no_grad():
                pb = torch.cat([tb(p.proposal_boxes) for p in proposals]).to(dev).float()
                gb = torch.cat([tb(p.gt_boxes) for p in proposals]).to(dev).float()
                gc = torch.cat([p.gt_classes for p in proposals]).to(dev).int()
                rois5 = torch.cat([torch.zeros((pb.shape[0], 1), device=dev), pb], 1)
            if torch.is_grad_enabled() and (scores.requires_grad or bbox.requires_grad):
                from .train_modules import _SupLossFn
                lv = _SupLossFn.apply(scores, bbox, self, dict(gc=gc, rois5=rois5, gb=gb))
                out["loss_cls"], out["loss_box_reg"] = lv[0], lv[1]
            else:
                with torch.no_grad():
                    out["loss_cls"] = ops.softmax_ce(scores.float().contiguous(), 0, k + 1, gc)[0]
                    out["loss_box_reg"] = ops.box_reg_loss(bbox.float().contiguous(), 0, k, gc, rois5, gb, self.bbox_reg_weights,
                                                           loss_type=self.box_reg_loss_type, beta=self.smooth_l1_beta)[0]
        if weak_predictions is not None:
            out.update(self.weak_detector_head.losses(weak_predictions, weak_proposals, weak_targets))
        return out

    def predict_probs(self, predictions, proposals):
        scores, _ = predictions
        return ops.softmax_rows(scores.float().contiguous(), self.num_classes + 1).split([len(p) for p in proposals], dim=0)

    @torch.no_grad()
    def inference(self, predictions, proposals, tta=False):
        """fast_rcnn.py:455-468 -> (list[Instances(pred_boxes, scores, pred_classes)], list[filter_inds]) (d2 fast_rcnn_inference:
        softmax, drop bg, apply_deltas, clip, score > thresh, per-class NMS, top-k) on the device"""
        if tta:
            raise NotImplementedError("TTA is outside the hot path (SURVEY.md section 2)")
        scores, bbox = predictions
        return _detect(self, ops.softmax_rows(scores.float().contiguous(), self.num_classes + 1), bbox, proposals)


@FAST_RCNN_REGISTRY.register()
class SupervisedDetectorOutputsFineTune(SupervisedDetectorOutputsBase):
    finetune = True

    # ---- a14: SupervisedDetectorOutputsFineTune.forward fast_rcnn.py:484-533 (scores/bbox assembled by
    # unit_transfer_predictions incl. the zero-initialised *_ft heads -- under REGRESSION_BRANCH by unit_transfer_predictions_ex, which adds the
    # weak head's box deltas in the same launch: `transfer` above; no -inf fill) + FastRCNNOutputs.losses
    def ft_losses(self, scores, bbox, roi_cls, rois5, roi_gt, loss_out, grad_dtype):
        """d(loss)/d(scores|bbox) == d(loss)/d([cls_score_ft | bbox_pred_ft] outputs): the ft heads enter additively."""
        k = self.num_classes
        dy = ops.zeros((scores.shape[0], self.group_ft.kp), grad_dtype, scores.device)
        ops.softmax_ce(scores, 0, k + 1, roi_cls, dy=dy, dcol0=self.col_cls, loss_out=loss_out[0:1])
        ops.box_reg_loss(bbox, 0, k, roi_cls, rois5, roi_gt, self.bbox_reg_weights, dy=dy, dcol0=self.col_bbox, loss_out=loss_out[1:2],
                         loss_type=self.box_reg_loss_type, beta=self.smooth_l1_beta)
        return dy
