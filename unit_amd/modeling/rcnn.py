"""WeaklySupervisedRCNNNoMeta -- the MI355X counterpart of /root/reference/modeling/meta_arch/rcnn.py:431-542
(training `forward` :433-491, `preprocess_image` :257-266, `inference` :493-542, `_postprocess` :411-429).
WeaklySupervisedRCNNRPN (:544-654; the end of this file) is the same model with the weak batch training the RPN through pseudo ground truth.

One training step = ONE explicit forward plan + ONE explicit backward plan over the HIP kernels (no autograd graph, no
host sync): `forward_train` saves exactly the activations the backward needs, `backward_train` walks them in reverse and
writes parameter gradients straight into the flat gradient buffer (unit_amd/flat.py). For drop-in use under a
Detectron2-style trainer (`loss_dict = model(data, weak_batched_inputs=...); sum(loss_dict.values()).backward()`,
engine/defaults.py:279-283) the plan is exposed to torch.autograd as a single Function node.

Batching: the supervised and the weak images of a step go through the backbone and the RPN head as ONE batch
(rcnn.py:439,452 run the backbone twice; same arithmetic per image), the supervised and weak RoIs go through RoIAlign
and `weak_box_head` as ONE batch (roi_heads.py:499-513).
"""
import contextlib
import os

import torch
from torch import nn

from .. import metrics as step_metrics
from .. import ops
from ..flat import FlatStore
from ..structures import (BACKBONE_REGISTRY, META_ARCH_REGISTRY, PROPOSAL_GENERATOR_REGISTRY, ROI_HEADS_REGISTRY, Boxes, ImageList,
                          Instances)

LOSS_NAMES = ["loss_cls", "loss_box_reg", "loss_im_cls", "loss_oicr_1", "loss_oicr_2", "loss_oicr_3", "loss_rpn_cls", "loss_rpn_loc",
              "loss_mask"]


class PackedBatch:
    """Device-resident, padded form of `batched_inputs` (+ weak) so that the step itself never touches the host."""

    def __init__(self, images, gt_boxes, gt_classes, gt_count, n_sup, multihot=None, gt_masks=None):
        self.images = images            # list of CHW fp32 device tensors: supervised first, then weak
        self.gt_boxes, self.gt_classes, self.gt_count = gt_boxes, gt_classes, gt_count
        self.n_sup = n_sup
        self.multihot = multihot        # [n_weak, K] uint8 or None
        self.gt_masks = gt_masks        # [n_sup, Mcap, H, W] uint8 bitmasks, structures.PackedPolygons (MASK_FORMAT "polygon"), or None

    @property
    def n_weak(self):
        return len(self.images) - self.n_sup

    def clone(self):
        """own copies of every buffer (the static inputs of a captured step must not alias the caller's tensors)"""
        c = lambda t: None if t is None else t.clone()
        return PackedBatch([im.clone() for im in self.images], c(self.gt_boxes), c(self.gt_classes), c(self.gt_count), self.n_sup,
                           c(self.multihot), c(self.gt_masks))

    def key(self):
        return (tuple(tuple(im.shape[-2:]) for im in self.images), self.n_sup, tuple(self.gt_boxes.shape), self.multihot is not None,
                None if self.gt_masks is None else tuple(self.gt_masks.shape))


def pack_gt_masks(ms, dev, mcap):
    """per-image ground-truth mask containers -> their device form: uint8 bitmasks [n, mcap, H, W] (Detectron2 BitMasks / plain tensors), or
    structures.PackedPolygons for PolygonMasks -- INPUT.MASK_FORMAT "polygon", what the reference's COCO-segm yaml trains on: the vertices
    travel to the device as they are and are rasterised inside each sampled box there (unit_mask_targets_polygon)"""
    if all(hasattr(m, "polygons") for m in ms):
        from ..structures import PackedPolygons
        return PackedPolygons.pack(ms, dev, mcap)
    ms = [m.tensor if hasattr(m, "tensor") else m for m in ms]
    hm, wm = max(m.shape[-2] for m in ms), max(m.shape[-1] for m in ms)
    gt_masks = torch.zeros((len(ms), mcap, hm, wm), dtype=torch.uint8)
    for i, m in enumerate(ms):
        gt_masks[i, : m.shape[0], : m.shape[-2], : m.shape[-1]] = m.to(torch.uint8).cpu() if m.is_cuda else m.to(torch.uint8)
    return gt_masks.to(dev, non_blocking=True)


def _rows(t, lo, hi):
    """t[lo:hi] of an optional per-RoI tensor (ROIPool's argmax buffer: None under the RoIAlign pooler types)"""
    return None if t is None else t[lo:hi]


class _StepFn(torch.autograd.Function):
    """Exposes the explicit plan to torch.autograd as one node: forward has already run, backward runs the backward plan."""

    @staticmethod
    def forward(ctx, anchor, model, step, loss_vec, used_mask=None):
        ctx.model, ctx.step, ctx.step_mask = model, step, used_mask
        return loss_vec.view_as(loss_vec)

    @staticmethod
    def backward(ctx, grad_losses):
        # every loss enters the total with weight 1 (engine/defaults.py:280 `sum(loss_dict.values())`): the backward plan has that
        # baked in, so a trainer that scales or drops losses (AMP GradScaler, loss weights, a subset of the dict) is refused rather
        # than silently given unscaled gradients. Losses the step did not produce are zero slots and may carry any weight.
        used = torch.ones_like(grad_losses, dtype=torch.bool) if ctx.step_mask is None else ctx.step_mask
        if not bool(torch.all(grad_losses[used] == 1.0)):
            raise RuntimeError("WeaklySupervisedRCNNNoMeta: backward() expects d(total)/d(loss_i) == 1 for every returned loss "
                               "(sum(loss_dict.values()).backward()); scaled / partial losses are not supported by the fused step")
        (ctx.model.backward_train_only_weak if getattr(ctx.step, "only_weak", False) else ctx.model.backward_train)(ctx.step)
        return torch.zeros(1, device=grad_losses.device), None, None, None, None


@META_ARCH_REGISTRY.register()
class WeaklySupervisedRCNNNoMeta(nn.Module):
    def __init__(self, cfg, thing_classes=None):
        super().__init__()
        self.cfg = cfg
        self.backbone = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg)
        shape = self.backbone.output_shape()
        self.proposal_generator = PROPOSAL_GENERATOR_REGISTRY.get(cfg.MODEL.PROPOSAL_GENERATOR.NAME)(cfg, shape)
        self.roi_heads = ROI_HEADS_REGISTRY.get(cfg.MODEL.ROI_HEADS.NAME)(cfg, shape, thing_classes)
        self.register_buffer("pixel_mean", torch.tensor(cfg.MODEL.PIXEL_MEAN).view(-1, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.tensor(cfg.MODEL.PIXEL_STD).view(-1, 1, 1), persistent=False)
        self._pixel_mean, self._pixel_std = list(cfg.MODEL.PIXEL_MEAN), list(cfg.MODEL.PIXEL_STD)
        self.normalize_images = cfg.INPUT.NORMALIZE_IMAGES
        self.num_classes = cfg.MODEL.ROI_HEADS.NUM_CLASSES
        for name, p in self.named_parameters():   # rcnn.py:250-255
            if any(layer == name.split(".")[0] for layer in cfg.MODEL.FREEZE_LAYERS.META_ARCH):
                p.requires_grad = False
        self._x3 = False
        self._compute_dtype = torch.bfloat16
        self.version = 0          # bumped by the optimizer: layers re-fold / re-cast their weights when it changes
        self.store = None
        self._anchor = None
        self._gen = None
        self.on_grad_ready = None  # data-parallel hook: called with a stage name as soon as its gradients are final
        self.on_bucket_final = None  # optimizer hook (tag, stream): the bucket's gradients are final once `stream` reaches this point
        self.use_multi_tensor_plan = True
        self.plan = None
        # opt-in (bench.py, TrainerNoMeta(overlap_tail=True)): the end of a step -- last gradient bucket's weight gradients, their
        # reduction, the data-parallel all-reduce waits, SGD, weight re-preparation -- stays on the weight-gradient stream and the NEXT
        # step's preprocessing / frozen stem / res2 run beside it; the main stream joins before its first trainable layer. Whoever reads
        # parameters or gradients on another stream in between calls join_optimizer_tail() first (state_dict() and inference do).
        self.overlap_optimizer_tail = False
        # ragged supervised / weak batches as ONE backbone + RPN-head pass (ops.Ragged: pointwise layers over the concatenated rows, every
        # other layer as a pair launch, weight gradients with the groups as parts): default; 0 = the two passes of rounds 1-4 (A/B, tests)
        self.ragged_single_pass = os.environ.get("UNIT_RAGGED", "1") != "0"
        self._tail_pending = None
        self.overlap_streams = True
        # opt-in (TrainerNoMeta(metrics=True)): the counts behind Detectron2's ten step scalars (unit_amd/metrics.py), added into one int32
        # vector by three small launches inside the step -- no sync; `last_metrics` = the last step's vector (None while the switch is off),
        # `last_metrics_images` = the number of supervised images it counted over
        self.collect_metrics = False
        self.last_metrics, self.last_metrics_images = None, 0

    @property
    def device(self):
        return self.pixel_mean.device

    # "bf16" (the benchmarked mode: bf16 activations, MFMA, fp32 accumulation), "fp32" (true fp32 MFMA: the parity mode, 1/16 of the MFMA
    # rate) or "bf16x3" (the parity-GRADE fast mode, csrc/split.hip: every conv with 64-multiple channel counts runs on the bf16 MFMA kernels
    # over split operands -- hi.Wh + hi.Wl + lo.Wh, ~2^-17 per product -- inside the fp32 plan: activations between convs are ops.X3 split
    # tensors, everything that is not a conv stays the fp32 kernel it is in the parity mode)
    @property
    def compute_mode(self):
        return "bf16x3" if self._x3 else ("bf16" if self._compute_dtype == torch.bfloat16 else "fp32")

    @compute_mode.setter
    def compute_mode(self, mode):
        assert mode in ("bf16", "fp32", "bf16x3"), mode
        from ..layers import set_x3
        self._compute_dtype = torch.bfloat16 if mode == "bf16" else torch.float32
        if self._x3 != (mode == "bf16x3"):
            self._x3 = mode == "bf16x3"
            set_x3(self, self._x3)

    # the torch dtype of the plan's activations / gradients (bf16x3: float32-typed). Assigning it selects the plain mode of that dtype.
    @property
    def compute_dtype(self):
        return self._compute_dtype

    @compute_dtype.setter
    def compute_dtype(self, dtype):
        self.compute_mode = "bf16" if dtype == torch.bfloat16 else "fp32"

    # ------------------------------------------------------------------ parameters
    def trainable_order(self):
        """(name, param) in the order gradients become final during backward (bucket order for data parallelism)."""
        rh, bp = self.roi_heads, self.roi_heads.box_predictor
        groups = []   # list of (tag, [(name, param, pad_after)], reserve_numel)

        def fused(tag, prefix, group):
            ws = [(f"{prefix}.{n}.weight", m.weight) for n, m in group]
            bs = [(f"{prefix}.{n}.bias", m.bias) for n, m in group]
            if not all(p.requires_grad for _, p in ws + bs):
                return
            lg_k = sum(m.weight.shape[0] for _, m in group)
            kp = (lg_k + 7) // 8 * 8
            cin = group[0][1].weight.shape[1]
            groups.append((tag, [(n, p, False) for n, p in ws], (kp - lg_k) * cin))
            groups.append((tag, [(n, p, False) for n, p in bs], 0))

        mh = getattr(rh, "mask_head", None)
        if mh is not None:
            members = [("predictor", mh.predictor)] + ([("predictor_delta", mh.predictor_delta)] if getattr(mh, "finetune", False) else [])
            if all(m.weight.requires_grad for _, m in members):
                fused("mask_head", "roi_heads.mask_head", members)
            else:       # fine-tune yaml: `predictor` frozen, `predictor_delta` trains (FREEZE_LAYERS.MASK_HEAD) -> plain slots
                for n, m in members:
                    if m.weight.requires_grad:
                        groups.append(("mask_head", [(f"roi_heads.mask_head.{n}.weight", m.weight, True),
                                                     (f"roi_heads.mask_head.{n}.bias", m.bias, True)], 0))
            if mh.deconv.weight.requires_grad:
                groups.append(("mask_head", [("roi_heads.mask_head.deconv.weight", mh.deconv.weight, True),
                                             ("roi_heads.mask_head.deconv.bias", mh.deconv.bias, True)], 0))
        if getattr(bp, "finetune", False):
            fused("heads", "roi_heads.box_predictor", [("cls_score_ft", bp.cls_score_ft), ("bbox_pred_ft", bp.bbox_pred_ft)])
        fused("heads", "roi_heads.box_predictor", [("cls_score_delta", bp.cls_score_delta), ("bbox_pred_delta", bp.bbox_pred_delta)])
        wh = bp.weak_detector_head
        fused("heads", "roi_heads.box_predictor.weak_detector_head",
              [("classifier_stream", wh.classifier_stream), ("detection_stream", wh.detection_stream)] +
              [(f"oicr_predictors.{i}", m) for i, m in enumerate(wh.oicr_predictors)] +
              ([("regression_branch_cls", wh.regression_branch_cls), ("regression_branch_bbox", wh.regression_branch_bbox)]
               if wh.regression_branch else []))          # (the order of wh.group: the head's fused master weight stays one view)

        def stage(tag, prefix, st):
            buckets = {}
            for i in range(len(st) - 1, -1, -1):
                b = st[i]
                k = st.bucket_of_block(i) if hasattr(st, "bucket_of_block") else 0
                for cn in ("conv3", "conv2", "conv1", "shortcut"):
                    c = getattr(b, cn)
                    if c is not None and c.weight.requires_grad:
                        buckets.setdefault(k, []).append((f"{prefix}.{i}.{cn}.weight", c.weight, True))
            for k in sorted(buckets):        # "res4", "res4.1", ...: in the order the backward completes them (layers.ResStage)
                groups.append((tag if k == 0 else f"{tag}.{k}", buckets[k], 0))

        stage("box_head", "roi_heads.box_head.res5", rh.box_head.res5)
        if rh.weak_box_head is not None:
            stage("weak_box_head", "roi_heads.weak_box_head.res5", rh.weak_box_head.res5)
        h = self.proposal_generator.rpn_head
        fused("rpn", "proposal_generator.rpn_head", [("objectness_logits", h.objectness_logits), ("anchor_deltas", h.anchor_deltas)])
        if h.conv.weight.requires_grad:
            groups.append(("rpn", [("proposal_generator.rpn_head.conv.weight", h.conv.weight, True),
                                   ("proposal_generator.rpn_head.conv.bias", h.conv.bias, True)], 0))
        stage("res4", "backbone.res4", self.backbone.res4)
        stage("res3", "backbone.res3", self.backbone.res3)
        stage("res2", "backbone.res2", self.backbone.res2)
        return groups

    def flatten_parameters(self):
        """Moves all trainable parameters into one flat fp32 buffer (+ flat grads); idempotent; call after .to(device)."""
        dev = self.device
        store = FlatStore(dev)
        store.tags = []   # (tag, start, end) ranges for the data-parallel buckets
        seen = set()
        for tag, items, reserve in self.trainable_order():
            start = store.size
            for name, p, pad_after in items:
                store.add(name, p, pad_after=pad_after)
                seen.add(id(p))
            if reserve:
                store.reserve(reserve)
            store.pad()
            store.tags.append((tag, start, store.size))
        missing = [n for n, p in self.named_parameters() if p.requires_grad and id(p) not in seen]
        if missing:
            raise RuntimeError(f"trainable parameters without a slot in the backward plan: {missing[:5]}")
        store.materialize()
        self.store = store
        self.version += 1
        from ..multi import ConvPlan
        self.plan = ConvPlan(self) if self.device.type == "cuda" and self.use_multi_tensor_plan else None
        return store

    def after_optimizer_step(self):
        """called by the optimizer once the flat parameters changed: bump the version and refresh every trainable conv's
        prepared (FrozenBN-folded, cast, dgrad-transposed) copies in one multi-tensor launch."""
        self.version += 1
        self._plan_ok_version = None
        if getattr(self, "plan", None) is not None and self.plan.prep_all(self.compute_dtype, self.version):
            self._plan_ok_version = self.version          # every planned conv's copies were refreshed by the multi-tensor launch

    def _ensure_ready(self):
        if self.training and (self.store is None or not self.store.is_current()):
            self.flatten_parameters()
        dt, v = self.compute_dtype, self.version
        pending = self._tail_pending is not None
        if pending and getattr(self, "_plan_ok_version", None) != v:
            # (first steps) per-layer weight preparation would read parameters the optimizer tail is still writing on its stream
            self.join_optimizer_tail()
            pending = False
        self.backbone.prepare(dt, v)
        if pending:
            # the Linear groups of the RPN / ROI heads re-prepare their weights from the parameters EVERY step (they are not in the conv
            # plan): with the previous step's update still running on the weight-gradient stream that happens in join_optimizer_tail(),
            # not here on the current stream beside it (a race the round-4 stream placement exposed: test_rccl_gpu tail_overlap)
            self._heads_unprepared = True
            return
        self.proposal_generator.rpn_head.prepare(dt, v)
        self.roi_heads.prepare(dt, v)

    # ------------------------------------------------------------------ inputs
    def pack_batch(self, batched_inputs, weak_batched_inputs=None, gt_capacity=None, gt_buckets=None):
        """gt_capacity: fixed number of GT slots per image (a multiple of 8, >= the largest image's count) -- static shapes for a
        captured step; gt_buckets: ascending capacities, the smallest one that holds the batch is taken (beyond the last: the next
        multiple of it); default: the batch's own maximum rounded up to 8"""
        dev = self.device
        sup = batched_inputs or []
        weak = weak_batched_inputs or []
        images = [x["image"].to(dev, non_blocking=True).float() for x in list(sup) + list(weak)]
        n = len(sup)
        gtb, gtc = [], []
        for x in sup:
            inst = x["instances"]
            b = inst.gt_boxes.tensor if hasattr(inst.gt_boxes, "tensor") else inst.gt_boxes
            gtb.append(b)
            gtc.append(inst.gt_classes)
        mcap = max([len(b) for b in gtb] + [1])
        mcap = (mcap + 7) // 8 * 8
        if gt_buckets:
            fit = [b for b in gt_buckets if b >= mcap]
            gt_capacity = fit[0] if fit else (mcap + gt_buckets[-1] - 1) // gt_buckets[-1] * gt_buckets[-1]
        if gt_capacity is not None:
            if gt_capacity % 8 != 0 or gt_capacity < mcap:
                raise ValueError(f"pack_batch: gt_capacity {gt_capacity} must be a multiple of 8 and hold the {mcap} ground-truth slots of this batch")
            mcap = gt_capacity
        gt_boxes = torch.zeros((max(n, 1), mcap, 4), dtype=torch.float32)
        gt_classes = torch.zeros((max(n, 1), mcap), dtype=torch.int64)
        for i in range(n):
            gt_boxes[i, : len(gtb[i])] = gtb[i].float().cpu() if gtb[i].is_cuda else gtb[i].float()
            gt_classes[i, : len(gtc[i])] = gtc[i].cpu() if gtc[i].is_cuda else gtc[i]
        gt_count = torch.tensor([len(b) for b in gtb] or [0], dtype=torch.int32)
        multihot = None
        if weak:
            multihot = torch.zeros((len(weak), self.num_classes), dtype=torch.uint8)
            for i, x in enumerate(weak):
                c = x["instances"].gt_classes if "instances" in x else x["gt_classes"]
                multihot[i, c.long().cpu()] = 1     # torch.unique(gt_classes) (weak_detector_fast_rcnn.py:203)
            multihot = multihot.to(dev, non_blocking=True)
        gt_masks = None
        if n > 0 and all(x["instances"].has("gt_masks") for x in sup):
            gt_masks = pack_gt_masks([x["instances"].gt_masks for x in sup], dev, mcap)
        return PackedBatch(images, gt_boxes.to(dev, non_blocking=True), gt_classes.to(dev, non_blocking=True),
                           gt_count.to(dev, non_blocking=True), n, multihot, gt_masks)

    def preprocess_image(self, batched_inputs):
        """rcnn.py:257-266 -> ImageList(NHWC tensor with channels padded to 8, image_sizes)."""
        imgs = [x["image"].to(self.device).float() if isinstance(x, dict) else x for x in batched_inputs]
        t, sizes = ops.preprocess_images(imgs, self._pixel_mean, self._pixel_std, self.compute_dtype, 8, self.normalize_images)
        return ImageList(t, sizes)

    def sampling_permutations(self, n_sup, n_anchor, n_roi_cap):
        """RNG for subsample_labels: one permutation per image and per sampler (explicit-permutation contract). Drawn on the
        device by unit_perm_keys + the stable sort from (SEED + rank, a device-resident step counter): no torch.randperm, no
        host state -- a captured step draws fresh permutations on every replay."""
        seed, counter = self._rng()
        rpn = ops.random_permutations(n_sup, n_anchor, seed, counter, 0, self.device)
        roi = ops.random_permutations(n_sup, n_roi_cap, seed, counter, 1, self.device)
        ops.counter_bump(counter)
        return {"rpn": rpn, "roi": roi}

    def _rng(self):
        """(SEED + rank, the device-resident step counter) behind every permutation draw"""
        if self._gen is None:
            seed = self.cfg.SEED if self.cfg.SEED >= 0 else 0
            rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
            self._gen = (seed + rank, torch.zeros(1, dtype=torch.int64, device=self.device))
        return self._gen

    # ------------------------------------------------------------------ the training step: forward plan
    def forward_train(self, batch, perms=None, early_backward=False, proposals=None):
        """-> step context (holds `losses` fp32[9] on the device and everything backward_train needs).
        early_backward: the caller WILL run backward_train right after (train_step / TrainerNoMeta.run_step); branches whose
        backward does not depend on later forward work (the RPN head) may then start during the forward plan.
        proposals: precomputed (boxes [B,P,4], objectness [B,P], count int32 [B]) for all images, supervised first -- the
        reference's `"proposals" in batched_inputs[0]` branch (rcnn.py:474-481); the RPN still trains on its own outputs."""
        self._ensure_ready()
        self._early_backward = early_backward
        if self.plan is not None:
            self.plan.begin_step()          # nothing a previous (interrupted) step queued may leak into this one
        rpn, rh, bp = self.proposal_generator, self.roi_heads, self.roi_heads.box_predictor
        dt = self.compute_dtype
        c = type("StepCtx", (), {})()
        n_sup, n_weak = batch.n_sup, batch.n_weak
        n_img = n_sup + n_weak
        c.n_sup, c.n_weak = n_sup, n_weak
        # (a subclass that has already written slots of this step's vector hands it over: WeaklySupervisedRCNNRPN)
        c.losses = self.__dict__.pop("_step_losses", None)
        if c.losses is None:
            c.losses = ops.zeros(len(self.loss_names), torch.float32, self.device)
        c.metrics = None
        if self.collect_metrics:
            c.metrics = ops.zeros(step_metrics.SIZE, torch.int32, self.device)          # (the library's own fill: a recorded call, replayed with the step)
        self.last_metrics, self.last_metrics_images = c.metrics, n_sup

        # a1 preprocess + a2 backbone. The reference runs the backbone once per batch (rcnn.py:439 supervised, :452 weak), each
        # batch zero-padded to ITS OWN largest image (ImageList.from_tensors). When both batches pad to the same size (always
        # the case for equally sized images, e.g. the benchmark) the two passes are arithmetically one batch of
        # n_sup + n_weak images and run as such; otherwise (`split`) they stay two passes, because a feature near the border
        # of the smaller padded tensor depends on where the zero padding of every conv layer starts.
        raw = [(int(im.shape[-2]), int(im.shape[-1])) for im in batch.images]
        pad_of = lambda ss: (max(s[0] for s in ss), max(s[1] for s in ss))
        split = n_sup > 0 and n_weak > 0 and pad_of(raw[:n_sup]) != pad_of(raw[n_sup:])
        c.split = split
        c.bb_ctx_w = None          # the weak batch's backbone context: the two-pass form of `split` only
        feat_w = head_w = anchors_w = feat_r = None
        if not split:
            x, sizes = ops.preprocess_images(batch.images, self._pixel_mean, self._pixel_std, dt, 8, self.normalize_images)
            feat, c.bb_ctx = self.backbone.fwd(x, save=True, before_trainable=self.join_optimizer_tail)
        else:
            xa, sa = ops.preprocess_images(batch.images[:n_sup], self._pixel_mean, self._pixel_std, dt, 8, self.normalize_images)
            xb, sb = ops.preprocess_images(batch.images[n_sup:], self._pixel_mean, self._pixel_std, dt, 8, self.normalize_images)
            sizes = sa + sb
            if self.ragged_single_pass:
                # ONE pass over both groups (ops.Ragged): the reference's two backbone calls (rcnn.py:439, :452) differ only in where each
                # batch's zero padding starts, which every non-pointwise layer gets from its group's own map size
                feat_r, c.bb_ctx = self.backbone.fwd([xa, xb], save=True, before_trainable=self.join_optimizer_tail)
                feat, feat_w = feat_r.groups()
            else:          # the two passes one after the other (side by side on two streams they gained nothing: DESIGN, retired switches)
                feat, c.bb_ctx = self.backbone.fwd(xa, save=True, before_trainable=self.join_optimizer_tail)          # `feat` = supervised images only
                feat_w, c.bb_ctx_w = self.backbone.fwd(xb, save=True)
            anchors_w = rpn.anchor_generator.grid(feat_w.shape[1], feat_w.shape[2])
        self.join_optimizer_tail()          # (a fully frozen backbone never called it)
        c.image_sizes = sizes
        # bf16x3 mode: the backbone hands over split tensors (ops.X3). The RPN's conv reads them as they are; RoIAlign, its backward and the
        # ReLU mask of the map gradient are fp32 kernels and read a merged copy (38 MB for four 600x1000 images) -- `feat` below
        feat_c, feat_w_c = feat, feat_w
        feat, feat_w = ops.as_f32(feat), (ops.as_f32(feat_w) if feat_w is not None else None)
        c.feat, c.feat_w = feat, feat_w
        n, fh, fw, fc = feat.shape
        anchors = rpn.anchor_generator.grid(fh, fw)

        # a3 RPN head on all images; a4/a5 labels + loss on the supervised ones; a6 proposals for all (no grad)
        n_roi_cap = rpn.post_nms_topk[True] + batch.gt_boxes.shape[1]
        # The RPN branch (anchor labelling -> loss -> backward) needs nothing from the proposal pipeline and vice versa: with
        # early_backward the whole branch runs on a side stream, so that its dense conv work fills the chip while the
        # latency-bound proposal chain (select -> rank sort -> decode -> NMS -> sampling, a few workgroups each) is the
        # only thing on the main stream's critical path.  The sampling permutations have no data dependence at all: they
        # are drawn on the side stream while the backbone is still running.
        side_rpn = (early_backward and n_sup > 0 and self._streams_on()
                    and any(p.requires_grad for p in rpn.rpn_head.parameters()))
        perm_ready = None
        if perms is None:
            if side_rpn:
                # fork first: work on a stream that has not joined the capturing stream would run at capture time instead of
                # being recorded (engine.GraphedStep); eagerly the draw just queues behind the backbone, off the critical path
                self._rpn_stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self._rpn_stream):
                    perms = self.sampling_permutations(n_sup, anchors.shape[0], n_roi_cap)
                    perm_ready = torch.cuda.Event()
                    perm_ready.record()
                perms["roi"].record_stream(torch.cuda.current_stream())
            else:
                perms = self.sampling_permutations(n_sup, anchors.shape[0], n_roi_cap)
        c.ragged = feat_r is not None
        if c.ragged:
            hr, c.rpn_ctx = rpn.rpn_head.fwd(feat_r, save=True)          # both groups: one conv launch, one predictor GEMM
            head, head_w = (hr.group(i).view(d[0], d[1] * d[2], hr.channels) for i, d in enumerate(hr.dims))
        else:
            head, c.rpn_ctx = rpn.rpn_head.fwd(feat_c, save=True)
            if split:
                head_w, _ = rpn.rpn_head.fwd(feat_w_c, save=False)          # weak images: proposals only (no RPN loss)
        c.dhead = None
        c.drpn = None
        c.rpn_bwd_early = False

        def rpn_branch():
            c.anchor_labels, c.anchor_match, _ = rpn.label_and_sample_anchors(anchors, batch.gt_boxes, batch.gt_count, perms["rpn"])
            if c.metrics is not None:
                ops.metrics_rpn(c.anchor_labels, c.metrics[step_metrics.RPN:step_metrics.RPN + 5])
            _, c.dhead = ops.rpn_loss(head[:n_sup], rpn.num_anchors, rpn.num_anchors, c.anchor_labels, c.anchor_match, batch.gt_boxes,
                                      anchors, rpn.batch_size_per_image * n_sup, dt, loss_out=c.rpn_losses,
                                      weights=(rpn.loss_weight["loss_rpn_cls"], rpn.loss_weight["loss_rpn_loc"]),
                                      loss_type=rpn.box_reg_loss_type, beta=rpn.smooth_l1_beta)

        if side_rpn:
            self._reattach_grads()
            main, s2 = torch.cuda.current_stream(), self._rpn_stream
            s2.wait_stream(main)
            for t in (head, feat, feat_c, anchors, perms["rpn"], c.losses) + tuple(c.rpn_ctx) + (() if c.metrics is None else (c.metrics,)):
                t.record_stream(s2)
            with torch.cuda.stream(s2):
                c.rpn_losses = c.losses[6:8]          # the branch writes its two slots of the loss vector itself; nobody else touches them
                rpn_branch()
                c.drpn = rpn.rpn_head.bwd(c.rpn_ctx, c.dhead, n_sup)
                if self.plan is not None:
                    # the 3x3 conv's weight gradient was queued for the heads' grouped launch, which goes out at the first bucket boundary
                    # of the backward plan -- behind everything this stream is given later (the OICR chains) and next to the predictors'
                    # backward. Launched here it runs under RoIAlign (HBM-bound, a few waves per CU) while the chip is half empty.
                    self.plan.launch_deferred()
                # what the backward plan waits for: this point of the stream, not whatever the stream is given later (OICR chains,
                # engine.EarlyUpdate's per-bucket optimizer launches)
                c.rpn_branch_done = torch.cuda.Event()
                c.rpn_branch_done.record()
            c.rpn_bwd_early = True
        elif n_sup > 0:
            c.rpn_losses = c.losses[6:8]
            rpn_branch()
        hw = self._sizes_on_device(sizes)
        if proposals is not None:
            props, pscores, pcount = proposals
        elif not split:
            props, pscores, pcount = rpn.predict_proposals(head, anchors, hw, True)
        else:          # two groups of anchors: the same call per group, one set of tensors
            post = rpn.post_nms_topk[True]
            props, pscores, pcount = split_props = (torch.empty((n_img, post, 4), dtype=torch.float32, device=self.device),
                                                    torch.empty((n_img, post), dtype=torch.float32, device=self.device),
                                                    torch.empty((n_img,), dtype=torch.int32, device=self.device))
            rpn.predict_proposals(head_w, anchors_w, hw[n_sup:], True, out=tuple(t[n_sup:] for t in split_props))
            rpn.predict_proposals(head, anchors, hw[:n_sup], True, out=tuple(t[:n_sup] for t in split_props))
        c.proposals = (props, pscores, pcount)
        if perm_ready is not None:
            torch.cuda.current_stream().wait_event(perm_ready)

        # a7 RoI sampling (supervised) + first-512 weak proposals ; a8 RoIAlign on all RoIs at once
        s = rh.batch_size_per_image
        c.roi_cls, c.roi_gt = None, None
        c.sw = sw = rh.weak_rows_per_image(props)          # (MODEL.LOAD_PROPOSALS: every proposal slot of a weak image)
        rs, rw = n_sup * s, n_weak * sw
        c.rois = torch.empty((rs + rw, 5), dtype=torch.float32, device=self.device)          # supervised RoIs, then weak: both samplers write their rows
        if n_sup > 0:
            _, c.roi_cls, c.roi_gt, c.roi_counts = rh.label_and_sample_proposals(props[:n_sup], pcount[:n_sup], batch.gt_boxes,
                                                                                 batch.gt_classes, batch.gt_count, perms["roi"],
                                                                                 rois_out=c.rois[:rs])
        if n_weak > 0:
            _, c.weak_valid = rh.weak_rois(props[n_sup:], pcount[n_sup:], n_sup, rois_out=c.rois[rs:])
        c.rs, c.rw = rs, rw
        if not split:          # (c.pool_argmax: POOLER_TYPE "ROIPool" leaves its selection beside `pooled` for the gather backward; else None)
            pooled, c.pool_argmax = rh.pool_train(feat, c.rois)
        else:   # two feature tensors, one pooled buffer: supervised RoIs from `feat`, weak RoIs (batch index rebased) from `feat_w`
            osz = rh.pool_out[0]
            pooled = torch.empty((rs + rw, osz, osz, fc), dtype=feat.dtype, device=feat.device)
            c.pool_argmax = rh.new_argmax(pooled)
            rh.pool(feat, c.rois[:rs], out=pooled[:rs], argmax=_rows(c.pool_argmax, 0, rs))
            rh.pool(feat_w, c.rois[rs:], out=pooled[rs:], image_offset=n_sup,          # (the RoIs' batch indices count from the supervised images)
                    argmax=_rows(c.pool_argmax, rs, rs + rw))

        # a9 Res5 heads: box_head on the supervised RoIs (grad); weak_box_head on ALL RoIs in one pass -- its supervised
        # half is the reference's no_grad evaluation (roi_heads.py:502-504), its weak half has grad (:512-513)
        multi = rh.weak_box_head is not None
        box_trainable = any(p.requires_grad for p in rh.box_head.parameters())
        c.head_overlap = False
        sup_rows_done = None
        c.weak_ctx_rows = slice(rs, rs + rw)         # rows of the weak RoIs inside weak_box_head's saved context
        if multi:
            if rs > 0 and self._streams_on() and getattr(rh, "mask_head", None) is None:
                # the two Res5 heads are independent: run box_head on its own HIP stream so that its workgroups fill the
                # tile-quantisation tails of weak_box_head's launches (and vice versa)
                main, s1 = torch.cuda.current_stream(), self._head_stream
                s1.wait_stream(main)
                pooled.record_stream(s1)
                with torch.cuda.stream(s1):
                    c.box_feat, c.box_ctx = rh.box_head.fwd(pooled[:rs], save=box_trainable)
                if rw > 0:
                    # three equal chains (box_head, weak_box_head on the supervised RoIs without saving, weak_box_head on the weak RoIs)
                    # on three streams instead of a 1 : 2 pair: they end together and their 392-tile launches pack into whole rounds
                    # ("three-chain head form")
                    s3 = self._wgrad_stream              # idle during the forward plan
                    s3.wait_stream(main)
                    pooled.record_stream(s3)
                    # both chains write their rows of ONE feature matrix (no concatenation afterwards)
                    wfeat_all = torch.empty((rs + rw, rh.weak_box_head.out_channels), dtype=pooled.dtype, device=pooled.device)
                    wfeat_all.record_stream(s3)
                    with torch.cuda.stream(s3):
                        f_sup, _ = rh.weak_box_head.fwd(pooled[:rs], save=False, feat_out=wfeat_all[:rs])
                        sup_rows_done = torch.cuda.Event()          # weak_box_head's features of the supervised RoIs are complete here
                        sup_rows_done.record()
                    f_weak, c.weak_ctx = rh.weak_box_head.fwd(pooled[rs:], save=True, feat_out=wfeat_all[rs:])
                    main.wait_stream(s3)
                    if f_sup.data_ptr() != wfeat_all.data_ptr() or f_weak.data_ptr() != wfeat_all[rs:].data_ptr():
                        f_sup.record_stream(main)          # (a head form without the fused pooling epilogue returned its own buffers)
                        wfeat_all = torch.cat([f_sup, f_weak], 0)
                        sup_rows_done = None
                    c.weak_ctx_rows = None               # the context covers exactly the weak RoIs
                else:
                    wfeat_all, c.weak_ctx = rh.weak_box_head.fwd(pooled, save=(rw > 0))
                main.wait_stream(s1)
                c.box_feat.record_stream(main)
                c.head_overlap = True
            else:
                c.box_feat, c.box_ctx = rh.box_head.fwd(pooled[:rs], save=box_trainable) if rs > 0 else (None, None)
                wfeat_all, c.weak_ctx = rh.weak_box_head.fwd(pooled, save=(rw > 0))
            sup_weak_feat, weak_feat = wfeat_all[:rs], wfeat_all[rs:]
        else:
            feat_all, c.box_ctx = rh.box_head.fwd(pooled, save=box_trainable)
            c.box_feat, weak_feat = feat_all[:rs], feat_all[rs:]
            sup_weak_feat, c.weak_ctx = c.box_feat, None
            wfeat_all = feat_all
        c.weak_feat = weak_feat

        # a16 mask head (roi_heads.py:691-710): un-pooled res5 map of the foreground RoIs -> deconv -> 1x1 -> mask BCE.
        # The sampler emits [fg..., bg...] per image, so the fg RoIs of image i are the first n_fg_i <= 128 slots of its block.
        c.mask_ctx = None
        c.dsim_mask = None
        c.ft_ctx = None          # (fine-tune step only)
        mh = getattr(rh, "mask_head", None)

        def run_mask(sim=None, roles=None):
            from .mask_head import gather_match_index, mask_targets
            fgc = rh.max_fg_per_image
            ymap = c.box_ctx[1]
            sidx, midx = rh._last_sampling
            gidx = gather_match_index(sidx, midx)
            sel = [slice(i * s, i * s + fgc) for i in range(n_sup)]
            # the first fgc slots of every image's block as dense tensors: one launch per field (four torch.cat of per-image slices before)
            x_fg = ops.gather_blocks(ymap, n_sup, s, fgc)
            cls_fg = ops.gather_blocks(c.roi_cls, n_sup, s, fgc)
            rois_fg = ops.gather_blocks(c.rois, n_sup, s, fgc)
            if hasattr(batch.gt_masks, "poly_start"):          # polygon ground truth (structures.PackedPolygons)
                from .mask_head import mask_targets_polygon
                tgt = mask_targets_polygon(batch.gt_masks, rois_fg, ops.gather_blocks(gidx, n_sup, s, fgc), cls_fg, rh.num_classes, mh.mask_size)
            else:
                tgt = mask_targets(batch.gt_masks, rois_fg, ops.gather_blocks(gidx, n_sup, s, fgc), cls_fg, rh.num_classes, mh.mask_size)
            kw = {}
            if sim is not None:      # similarity['seg'][fg] (roi_heads.py:893-897): fg slot -> its RoI row
                rows = self._const_on_device(("fg_rows", n_sup, s, fgc), lambda: torch.cat([torch.arange(sl.start, sl.stop, dtype=torch.int32) for sl in sel]))
                c.dsim_mask = torch.zeros(sim.shape, dtype=torch.float32, device=self.device)
                kw = dict(sim=sim, sim_rows=rows, roles=roles, dsim=c.dsim_mask)
            if c.metrics is not None:          # (counted by the base mask head only: mask_head.fwd_train)
                kw["metrics"] = c.metrics[step_metrics.MASK:step_metrics.MASK + 5]
            c.mask_ctx = (mh.fwd_train(x_fg, cls_fg, tgt, c.losses[8:9], dt, **kw), sel)

        mask_now = mh is not None and rs > 0 and batch.gt_masks is not None
        if mask_now and not rh.finetune:
            run_mask()

        # a10-a12 predictors + losses (+ gradients w.r.t. the Linear outputs)
        lin_sup = lin_weak_sup = None
        if rs > 0 and rw > 0 and c.head_overlap and not getattr(bp, "finetune", False):
            # box_head's features were produced on the head stream and its losses will run there: the supervised predictors' GEMM goes there
            # too, at once, instead of queueing behind the weak predictors' on this stream (two 16- / 32-workgroup launches of ~25 us each)
            with torch.cuda.stream(self._head_stream):
                lin_sup = bp.group.fwd(c.box_feat)
                if sup_rows_done is not None and not torch.cuda.is_current_stream_capturing():
                    # (eager launches only: hipStreamEndCapture of ROCm 7.2 segfaults on the capture of this cross-stream event wait)
                    # three-chain form: the weak predictors' outputs on the SUPERVISED RoIs (the OICR columns that feed the supervised scores)
                    # need the chain on the weight-gradient stream only -- with them computed here, the supervised losses and box_head's
                    # backward (backward_train: `early_sup`) no longer wait for weak_box_head's pass over the weak RoIs on the main stream,
                    # the longest of the three
                    self._head_stream.wait_event(sup_rows_done)
                    lin_weak_sup = bp.weak_detector_head.group.fwd(wfeat_all[:rs])
        decoupled = lin_weak_sup is not None
        if decoupled:
            lin_weak_w = bp.weak_detector_head.group.fwd(wfeat_all[rs:])
        else:
            lin_weak_all = bp.weak_detector_head.group.fwd(wfeat_all)            # [rs+rw, 104] (oicr cols feed the sup scores)
            lin_weak_sup, lin_weak_w = lin_weak_all[:rs], lin_weak_all[rs:]
        c.dy_sup = c.dy_weak = None
        c.sup_losses_on_head_stream = False
        sup_side = None
        if rs > 0:
            if lin_sup is None:
                lin_sup = bp.group.fwd(c.box_feat)
            if getattr(bp, "finetune", False):
                # a14 (roi_heads.py:595-644 / :826-870 + fast_rcnn.py:484-533): similarity transfer is active in TRAINING too
                from .inference import class_roles, similarity_dict
                frozen = not any(p.requires_grad for n, p in bp.named_parameters() if not n.split(".")[0].endswith("_ft"))
                assert frozen, "fine-tune step: the delta / weak predictors must be frozen (FREEZE_LAYERS.FAST_RCNN of every *-ft.yaml)"
                wh = bp.weak_detector_head
                lin_ft = bp.group_ft.fwd(c.box_feat)
                c.lin_w_box = wh.group.fwd(c.box_feat)
                sims, lingual, keys = similarity_dict(self, c.lin_w_box, want_ctx=True)
                t = class_roles(self)
                # (REGRESSION_BRANCH: lin_weak_sup holds the regression columns; unit_transfer_predictions_ex adds both in this one launch)
                c.scores, bbox = bp.transfer(lin_sup, lin_weak_sup, sims["cls"], sims["bbox"], t, ft=lin_ft)
                c.dy_sup = bp.ft_losses(c.scores, bbox, c.roi_cls, c.rois[:rs], c.roi_gt, c.losses[0:2], dt)
                if c.metrics is not None:          # on the transferred logits, as the reference's FastRCNNOutputs sees them
                    ops.metrics_fastrcnn(c.scores, 0, rh.num_classes + 1, c.roi_cls, c.metrics[step_metrics.FAST_RCNN:step_metrics.FAST_RCNN + 5])
                c.ft_ctx = (lin_sup, sims, lingual, keys, t)
                if mask_now and rh.finetune:        # WSROIHeadWithMaskFineTune hands similarity['seg'][fg] to the mask head
                    run_mask(sims.get("seg"), t)
            else:
                # the supervised losses (5 small launches) do not depend on the weak chain: they run on the head stream beside it
                sup_side = self._head_stream if (rw > 0 and self._streams_on()) else None
                if sup_side is not None and not decoupled:
                    sup_side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(sup_side) if sup_side is not None else contextlib.nullcontext():
                    c.dy_sup, c.scores = bp.sup_losses(lin_sup, lin_weak_sup, c.roi_cls, c.rois[:rs], c.roi_gt, c.losses[0:2], dt)
                    # behind the losses, on their stream: no edge of its own, but the join below that the main chain already makes for
                    # the losses (wait_stream(sup_side)) now waits for this launch too (a few microseconds)
                    if c.metrics is not None:
                        if sup_side is not None:
                            c.metrics.record_stream(sup_side)
                        ops.metrics_fastrcnn(c.scores, 0, rh.num_classes + 1, c.roi_cls, c.metrics[step_metrics.FAST_RCNN:step_metrics.FAST_RCNN + 5])
                c.sup_losses_on_head_stream = sup_side is not None
        if rw > 0:
            # REGRESSION_BRANCH: the weak head's two further losses take the slots behind LOSS_NAMES (self.loss_names)
            reg_kw = dict(reg_loss_out=c.losses[len(LOSS_NAMES):]) if bp.weak_detector_head.regression_branch else {}
            c.dy_weak = bp.weak_detector_head.fused_losses(lin_weak_w, c.rois[rs:], c.weak_valid, c.sw, n_weak,
                                                     batch.multihot, c.losses[2:6], dt,
                                                     side_stream=self._rpn_stream if self._streams_on() else None, **reg_kw)
        if sup_side is not None:
            torch.cuda.current_stream().wait_stream(sup_side)
        return c

    # ------------------------------------------------------------------ the training step: backward plan
    def backward_train(self, c):
        rpn, rh, bp = self.proposal_generator, self.roi_heads, self.roi_heads.box_predictor
        dt = self.compute_dtype
        self._reattach_grads()
        rs, rw, n_sup = c.rs, c.rw, c.n_sup
        multi = rh.weak_box_head is not None
        hook, plan = self.on_grad_ready, self.plan

        side = self._wgrad_stream if self._streams_on() else None
        ops.WGRAD_STREAM = side if plan is not None else None

        final = self.on_bucket_final

        def done(tag):
            if side is not None:
                # the bucket's wgrad kernels ran on the side stream: reduce its slabs (and launch its all-reduce) THERE, so
                # that the main stream's dgrad chain never waits for weight gradients; the streams join before the optimizer
                if hook is not None or final is not None:
                    side.wait_stream(torch.cuda.current_stream())      # bias / Linear gradients of the bucket come from main
                with torch.cuda.stream(side):
                    plan.reduce(tag)     # split-M slabs of this bucket -> flat gradient buffer (one launch)
                    if hook is not None:
                        hook(tag)        # data parallel: launch the bucket's all-reduce
                if final is not None:
                    final(tag, side)     # the bucket's gradients are final once `side` gets here: its optimizer update may start
                return
            if plan is not None:
                plan.reduce(tag)
            if hook is not None:
                hook(tag)

        feat = c.feat
        bb_trainable = self.backbone.first_trainable_stage() < 3
        box_trainable = c.box_ctx is not None
        # A step without a weak (or without a supervised) batch produces no gradient for the heads that only that batch feeds. torch
        # leaves such parameters' .grad at None and SGD skips them (weight decay included); here every gradient lives in the flat
        # buffer the optimizer sweeps, so those ranges are cleared instead of carrying the previous step's values into the update
        # (and, data parallel, into another all-reduce).
        if c.dy_weak is None or c.dy_sup is None:
            self._clear_unproduced(c)

        dbox = dweak = dall_buf = None
        # overlap: the two Res5 heads' backward as two chains, box_head's on the head stream. Requires that the forward ran them that way
        # (c.head_overlap: two heads, streams on, no mask head), that box_head trains and that both RoI groups produced a gradient.
        overlap = c.head_overlap and box_trainable and c.dy_sup is not None and c.dy_weak is not None
        # early_sup: the supervised predictors' backward already runs on the head stream, behind the supervised losses that ran there beside
        # the (three times longer) weak loss chain on this one, so box_head's backward starts ~0.3 ms before weak_box_head's, while only one-
        # and two-workgroup loss kernels run (profiles/r04_exp_head_backward_start.txt). Requires `overlap`, the losses on the head stream
        # (never in a fine-tune step) and eager launches (a captured segment must fork the head stream itself).
        early_sup = overlap and c.sup_losses_on_head_stream and not torch.cuda.is_current_stream_capturing()
        if c.dy_sup is not None and getattr(bp, "finetune", False):
            # VOC fine-tune yaml: everything below the ft heads is frozen -> their weight gradients are all there is.
            # COCO segm fine-tune yaml: the box head (and RPN) train -> the gradient continues through the ft heads, the frozen
            # delta heads incl. the base->novel transfer, and the similarity (computed WITH grad in the reference, roi_heads.py:852)
            # into the box head's features.
            dbox = bp.group_ft.bwd(c.box_feat, c.dy_sup, need_dx=box_trainable)
            if box_trainable:
                from .inference import similarity_backward
                lin_sup, sims, lingual, keys, t = c.ft_ctx
                wh = bp.weak_detector_head
                dlin, dsim = ops.transfer_predictions_bwd(c.dy_sup, bp.col_cls, bp.col_bbox, lin_sup, bp.col_cls, bp.col_bbox, rh.num_classes,
                                                          sims["cls"], sims["bbox"], t, bp.group.kp)
                if c.dsim_mask is not None:
                    dsim += c.dsim_mask
                dlin_w = similarity_backward(rh, c.lin_w_box, lingual, keys, dsim, dt)          # (one matrix for all heads: asserted there)
                dbox = dbox + bp.group.bwd(c.box_feat, dlin, need_dx=True) + wh.group.bwd(c.box_feat, dlin_w, need_dx=True)
        elif c.dy_sup is not None:
            if early_sup:
                with torch.cuda.stream(self._head_stream):
                    dbox = bp.group.bwd(c.box_feat, c.dy_sup, need_dx=True)
                    sup_pred_done = torch.cuda.Event()
                    sup_pred_done.record()
            else:
                if not multi and c.dy_weak is not None and box_trainable:
                    # one Res5 head serves both RoI groups (MULTI_BOX_HEAD False): the two predictors' input gradients are the rows of ONE
                    # matrix, written in place (a torch.cat before)
                    dall_buf = torch.empty((rs + rw, c.box_feat.shape[1]), dtype=c.dy_sup.dtype, device=self.device)
                dbox = bp.group.bwd(c.box_feat, c.dy_sup, need_dx=box_trainable or bb_trainable, out=dall_buf[:rs] if dall_buf is not None else None)
        if c.dy_weak is not None:
            dweak = bp.weak_detector_head.group.bwd(c.weak_feat, c.dy_weak, need_dx=True, out=dall_buf[rs:] if dall_buf is not None else None)
        if early_sup:
            torch.cuda.current_stream().wait_event(sup_pred_done)      # the bucket's gradients are complete on this stream's timeline
        done("heads")
        dpool_sup = dpool_weak = None      # d(loss)/d(pooled) of the supervised / weak RoIs
        mask_hook = None
        if c.mask_ctx is not None:
            mh = rh.mask_head

            def mask_hook(g, y):
                """adds the mask head's gradient to the res5 map gradient of the fg RoI slots (deconv dgrad with the
                running gradient as residual and the ReLU mask of the map as epilogue, written in place)."""
                ctx, sel = c.mask_ctx
                dy1 = mh.bwd(ctx)
                fgc = rh.max_fg_per_image
                for i, sl in enumerate(sel):
                    mh.deconv.dgrad(dy1[i * fgc:(i + 1) * fgc], residual=g[sl], mask_ref=y[sl], out=g[sl])
                done("mask_head")
        if multi:
            if overlap:
                main, s1 = torch.cuda.current_stream(), self._head_stream
                if not early_sup:
                    s1.wait_stream(main)
                    dbox.record_stream(s1)
                with torch.cuda.stream(s1):
                    dpool_sup = rh.box_head.bwd(c.box_ctx, dbox)
                dpool_weak = rh.weak_box_head.bwd(c.weak_ctx, dweak, row_slice=c.weak_ctx_rows)
                main.wait_stream(s1)
                dpool_sup.record_stream(main)
                done("box_head")
                done("weak_box_head")
            else:
                if dbox is not None and box_trainable:
                    dpool_sup = rh.box_head.bwd(c.box_ctx, dbox, map_grad_hook=mask_hook)
                    done("box_head")
                if dweak is not None:
                    dpool_weak = rh.weak_box_head.bwd(c.weak_ctx, dweak, row_slice=c.weak_ctx_rows)
                    done("weak_box_head")
        else:
            parts = [t for t in (dbox, dweak) if t is not None]
            if parts and box_trainable:
                dall = dall_buf if (dall_buf is not None and len(parts) == 2) else (torch.cat(parts, 0) if len(parts) > 1 else parts[0])
                dpool = rh.box_head.bwd(c.box_ctx, dall, map_grad_hook=mask_hook)
                done("box_head")
                dpool_sup, dpool_weak = (dpool[:rs] if rs > 0 else None), (dpool[rs:] if rw > 0 else None)

        drpn = None
        if c.rpn_bwd_early:
            torch.cuda.current_stream().wait_event(c.rpn_branch_done)      # launched during the forward plan
            if side is not None:
                side.wait_event(c.rpn_branch_done)                         # its wgrad slabs are reduced on the side stream
            drpn = c.drpn
            drpn.record_stream(torch.cuda.current_stream())
            c.rpn_losses.record_stream(torch.cuda.current_stream())
            # (the branch wrote loss_rpn_cls / loss_rpn_loc into its slots of c.losses)
            done("rpn")
        elif c.dhead is not None and any(p.requires_grad for p in rpn.rpn_head.parameters()):
            drpn = rpn.rpn_head.bwd(c.rpn_ctx, c.dhead, n_sup)
            done("rpn")
        if bb_trainable:
            # (bf16x3 mode: the Res5 heads and the RPN conv return split tensors, the RoIAlign backward is an fp32 kernel)
            dpool_sup, dpool_weak, drpn = ops.as_f32(dpool_sup), ops.as_f32(dpool_weak), ops.as_f32(drpn)
            # d(loss)/d(res4 output) = RoIAlign backward (gather form, deterministic) + RPN branch, times the ReLU mask --
            # one fused kernel per image group (supervised RoIs only touch supervised images, weak RoIs weak images)
            def grad_map(ft, dp, n_im, r_lo, r_hi, img0, add, out=None):
                out = out if out is not None else torch.empty_like(ft)
                if dp is not None:
                    rh.pool_bwd_gather(dp, n_im, ft.shape[1], ft.shape[2], c.rois[r_lo:r_hi], out, image_offset=img0, addend=add, mask_ref=ft,
                                       argmax=_rows(c.pool_argmax, r_lo, r_hi))
                else:
                    ops.add_cast(ops.zeros(ft.shape, torch.float32, ft.device), add, dt, mask_ref=ft, out=out)
                return out

            if not c.split:
                g = torch.empty_like(feat)
                n_img, fh, fw, _ = feat.shape
                for (dp, lo, hi, r_lo, r_hi, add) in ((dpool_sup, 0, n_sup, 0, rs, drpn), (dpool_weak, n_sup, n_img, rs, rs + rw, None)):
                    if hi <= lo:
                        continue
                    if dp is not None:
                        rh.pool_bwd_gather(dp, hi - lo, fh, fw, c.rois[r_lo:r_hi], g[lo:hi], image_offset=lo, addend=add,
                                           mask_ref=feat[lo:hi], argmax=_rows(c.pool_argmax, r_lo, r_hi))
                    else:
                        z = ops.zeros(feat[lo:hi].shape, torch.float32, feat.device)
                        ops.add_cast(z, add, dt, mask_ref=feat[lo:hi], out=g[lo:hi])
                self.backbone.bwd(c.bb_ctx, g, on_stage_done=done)
            elif c.ragged:
                # ragged batches, single pass: the two groups' gradient maps are the rows of ONE ops.Ragged; one backward pass
                gr = ops.Ragged.empty([tuple(feat.shape[:3]), tuple(c.feat_w.shape[:3])], feat.shape[3], feat)
                grad_map(feat, dpool_sup, n_sup, 0, rs, 0, drpn, out=gr.group(0))
                grad_map(c.feat_w, dpool_weak, c.n_weak, rs, rs + rw, n_sup, None, out=gr.group(1))
                self.backbone.bwd(c.bb_ctx, gr, on_stage_done=done)
            else:
                # ragged batches (forward ran the backbone twice): two backward passes; the weight gradients of the second
                # accumulate onto the first (whose slabs are reduced before the second pass may touch the same gradients)
                g_sup = grad_map(feat, dpool_sup, n_sup, 0, rs, 0, drpn)
                self.backbone.bwd(c.bb_ctx, g_sup, on_stage_done=None)
                if plan is not None:
                    if side is not None:
                        with torch.cuda.stream(side):
                            plan.reduce()
                    else:
                        plan.reduce()
                g_weak = grad_map(c.feat_w, dpool_weak, c.n_weak, rs, rs + rw, n_sup, None)
                ops.WGRAD_ACCUMULATE = True
                try:
                    self.backbone.bwd(c.bb_ctx_w, g_weak, on_stage_done=done)
                finally:
                    ops.WGRAD_ACCUMULATE = False
        if side is not None:
            if self.overlap_optimizer_tail and not torch.cuda.is_current_stream_capturing():
                side.wait_stream(torch.cuda.current_stream())      # the optimizer needs every gradient the main stream produced
                self._tail_pending = side
            else:
                torch.cuda.current_stream().wait_stream(side)
        ops.WGRAD_STREAM = None

    def high_priority_stream(self):
        """a HIGH-PRIORITY HIP stream to run the training steps on (`torch.cuda.set_stream(model.high_priority_stream())` once, as
        bench.py and TrainerNoMeta(high_priority=True) do): the step's main chain -- forward, dgrad chain, optimizer -- then outranks the
        side streams the plan forks (weight gradients, Res5 head chains, RPN branch; HIP has two levels, normal and high: the side
        streams cannot be lowered instead), so the dispatcher serves the critical chain's workgroups first whenever CUs free up.
        Measured: 16.31 -> 16.14 and 16.57 -> 16.47 ms per step in two alternating series, 123.5 vs 123.5 images/s in a third: at most the
        noise of the measurement, so nothing turns it on by default. NOT a per-step context: an event wait on PyTorch's default (null)
        stream per step costs the host its run-ahead (19.0 instead of 16.2 ms per step, measured)."""
        hp = self.__dict__.get("_step_hp_stream")
        if hp is None:
            hp = self.__dict__["_step_hp_stream"] = torch.cuda.Stream(self.device, priority=-1)
        return hp

    @contextlib.contextmanager
    def optimizer_tail(self):
        """stream context for what follows backward_train() in a step (GradBuckets.finish, FlatSGD.step enter it themselves): the
        weight-gradient stream while a tail is pending (overlap_optimizer_tail), the current stream otherwise"""
        s = self._tail_pending
        if s is None:
            yield
        else:
            with torch.cuda.stream(s):
                yield

    def join_optimizer_tail(self):
        """the current stream waits for a pending optimizer tail (no-op without one)"""
        s = self._tail_pending
        if s is not None:
            torch.cuda.current_stream().wait_stream(s)
            self._tail_pending = None
        if self.__dict__.get("_heads_unprepared"):
            self._heads_unprepared = False
            self.proposal_generator.rpn_head.prepare(self.compute_dtype, self.version)
            self.roi_heads.prepare(self.compute_dtype, self.version)

    def state_dict(self, *args, **kwargs):
        self.join_optimizer_tail()
        return super().state_dict(*args, **kwargs)

    def _const_on_device(self, key, make):
        """small host-built constants of the step (image sizes, slot tables) are uploaded once per distinct value: no pageable
        host-to-device copy inside the step -- which a hipGraph capture of the step could not contain"""
        cache = self.__dict__.setdefault("_dev_consts", {})
        t = cache.pop(key, None)
        if t is None or t.device != self.device:
            # bounded: evaluating a dataset of varied image sizes meets a new (sizes, output sizes) combination per batch.
            # Least-recently-USED eviction; once captured graphs / recorded call lists may hold an entry's address, an evicted tensor is
            # parked like an outgrown workspace instead of being freed (the anchor grids: rpn.DefaultAnchorGenerator.grid)
            if len(cache) >= self.CONST_CACHE_CAP:
                old = cache.pop(next(iter(cache)))
                if ops._GRAPHS_ALIVE[0]:
                    ops._WS_RETIRED.append(old)
            t = make().to(self.device)
        cache[key] = t          # (re-)inserted at the back: most recently used
        return t

    CONST_CACHE_CAP = 256          # entries are a few bytes to a few KB each

    def _sizes_on_device(self, sizes):
        return self._const_on_device(("hw", tuple(sizes)), lambda: torch.tensor(sizes, dtype=torch.float32))

    def _unfed_modules(self, has_sup, has_weak):
        """the modules whose parameters no loss of a step reaches: a pure function of which batches the step has and of MULTI_BOX_HEAD"""
        rh, bp = self.roi_heads, self.roi_heads.box_predictor
        mods = []
        if not has_weak:
            mods += list(bp.weak_detector_head.group.members)          # both streams, the refinement predictors, the regression branch
            if rh.weak_box_head is not None:
                mods.append(rh.weak_box_head)
        if not has_sup:
            mods += [bp.cls_score_delta, bp.bbox_pred_delta, self.proposal_generator.rpn_head] + \
                    ([bp.cls_score_ft, bp.bbox_pred_ft] if getattr(bp, "finetune", False) else [])
            if rh.weak_box_head is not None:
                mods.append(rh.box_head)          # (single-head configurations: box_head also serves the weak RoIs)
        return mods

    def _clear_unproduced(self, c):
        for m in self._unfed_modules(c.dy_sup is not None, c.dy_weak is not None):
            for p in m.parameters():
                if p.requires_grad and p.grad is not None:
                    p.grad.zero_()

    # ------------------------------------------------------------------ the weak-only step (train_only_weak=True, TrainerOnlyWeak)
    # A plan of its own beside forward_train / backward_train, which stay as they are: the reference's meta_arch/rcnn.py:437-491 with
    # batched_inputs=None is a short chain -- backbone (with gradient), RPN forward-only, first-k RoIs, RoIAlign, one Res5 head, the weak
    # detector's fused losses -- and none of the default plan's forks (RPN branch, two head chains, supervised losses) exists in it.
    only_weak_refused = None          # a meta-architecture that cannot take the mode says why (WeaklySupervisedRCNNRPN)

    def live_entries(self, has_sup, has_weak):
        """one bool per TRAINABLE entry of the flat store, in `store.entries` order (the rows of solver.clip_table): does a step with /
        without a supervised and a weak batch produce a gradient for it? False = torch leaves the parameter's .grad at None and
        torch.optim.SGD skips it. The same module lists `_clear_unproduced` zeroes; frozen stages have no entry at all."""
        if self.store is None or not self.store.is_current():
            self.flatten_parameters()
        dead = {id(p) for m in self._unfed_modules(has_sup, has_weak) for p in m.parameters()}
        return tuple(id(e["param"]) not in dead for e in self.store.entries if e["param"].requires_grad)

    def only_weak_tag_sequence(self):
        """the gradient buckets in the order the weak-only backward reports them: the ones a loss reaches as they become final (the order of
        `store.tags`), then the dead ones -- every tag once, whatever the mode, so a data-parallel rank never waits for a bucket that was
        not announced"""
        live = self.live_entries(False, True)
        ents = [e for e in self.store.entries if e["param"].requires_grad]
        fed = {}
        for tag, a, b in self.store.tags:
            fed[tag] = fed.get(tag, False) or any(l and a <= e["offset"] < b for l, e in zip(live, ents))
        return [t for t in fed if fed[t]] + [t for t in fed if not fed[t]]

    @property
    def only_weak_loss_names(self):
        """the keys of the mode's dictionary (rcnn.py:466-467, fast_rcnn.py `losses(..., train_only_weak=True)`): no RPN losses, no
        supervised losses -- the weak head's alone"""
        sup = ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc", "loss_mask")
        return [n for n in self.loss_names if n not in sup]

    def _check_only_weak(self, batch):
        """train_only_weak=True: what the reference's own code cannot run in this mode is refused with the line that stops it"""
        from .inference import UnsupportedConfig
        from .roi_heads import WSROIHeadNoMetaWithMask
        rh = self.roi_heads
        if self.only_weak_refused:
            raise NotImplementedError(self.only_weak_refused)
        if batch.n_sup > 0:
            raise NotImplementedError(ONLY_WEAK_WITH_SUPERVISED)
        if batch.n_weak == 0:
            raise ValueError("train_only_weak=True needs weak_batched_inputs (roi_heads.py:526: the box predictor would be called on None, None)")
        if isinstance(rh, WSROIHeadNoMetaWithMask):          # (and its fine-tune subclass)
            raise UnsupportedConfig(ONLY_WEAK_MASK_HEAD.format(type(rh).__name__))
        if getattr(rh, "finetune", False):
            raise UnsupportedConfig(ONLY_WEAK_FINETUNE.format(type(rh).__name__))
        if self._x3:
            raise NotImplementedError(ONLY_WEAK_X3)

    def forward_train_only_weak(self, batch):
        """-> step context of a batch of weak images alone (`losses` on the device, everything backward_train_only_weak needs). No sampling
        permutation is drawn, no anchor or RoI is labelled, nothing of the RPN head is saved for a backward (rcnn.py:468-470: no_grad)."""
        self._check_only_weak(batch)
        self._ensure_ready()
        if self.plan is not None:
            self.plan.begin_step()
        rpn, rh, wh = self.proposal_generator, self.roi_heads, self.roi_heads.box_predictor.weak_detector_head
        dt = self.compute_dtype
        c = type("StepCtx", (), {})()
        c.n_sup, c.n_weak, c.only_weak, c.split, c.mask_ctx = 0, batch.n_weak, True, False, None
        c.losses = ops.zeros(len(self.loss_names), torch.float32, self.device)
        c.metrics = ops.zeros(step_metrics.SIZE, torch.int32, self.device) if self.collect_metrics else None
        self.last_metrics, self.last_metrics_images = c.metrics, 0          # (no supervised image: no rpn/*, roi_head/*, fast_rcnn/* scalar)
        x, sizes = ops.preprocess_images(batch.images, self._pixel_mean, self._pixel_std, dt, 8, self.normalize_images)
        feat, c.bb_ctx = self.backbone.fwd(x, save=True, before_trainable=self.join_optimizer_tail)          # with gradient (:452)
        self.join_optimizer_tail()
        c.image_sizes = sizes
        c.feat = ops.as_f32(feat)
        _, fh, fw, _ = c.feat.shape
        head, _ = rpn.rpn_head.fwd(feat, save=False)
        c.proposals = props, _, pcount = rpn.predict_proposals(head, rpn.anchor_generator.grid(fh, fw), self._sizes_on_device(sizes), True)
        sw = rh.weak_rows_per_image(props)          # roi_heads.py:566-572: the first proposals of every image (all of them: LOAD_PROPOSALS)
        c.rs, c.rw = 0, batch.n_weak * sw
        c.rois, c.weak_valid = rh.weak_rois(props, pcount, 0)
        pooled, c.pool_argmax = rh.pool_train(c.feat, c.rois)
        c.head = rh.weak_box_head if rh.weak_box_head is not None else rh.box_head          # :512-515
        c.weak_feat, c.head_ctx = c.head.fwd(pooled, save=True)
        lin = wh.group.fwd(c.weak_feat)
        reg_kw = dict(reg_loss_out=c.losses[len(LOSS_NAMES):]) if wh.regression_branch else {}
        c.dy_weak = wh.fused_losses(lin, c.rois, c.weak_valid, sw, batch.n_weak, batch.multihot, c.losses[2:6], dt,
                                    side_stream=self._rpn_stream if self._streams_on() else None, **reg_kw)
        return c

    def backward_train_only_weak(self, c):
        """the weak head's predictors, its Res5 head, RoIAlign and the backbone in reverse; the ranges no loss reaches are cleared by the
        library's own fill and EVERY gradient bucket is reported final -- the fed ones as they complete, then the dead ones, which travel
        as the zeros they hold: the data-parallel schedule does not depend on the mode"""
        rh, wh = self.roi_heads, self.roi_heads.box_predictor.weak_detector_head
        self._reattach_grads()
        hook, plan, final = self.on_grad_ready, self.plan, self.on_bucket_final
        side = self._wgrad_stream if self._streams_on() else None
        ops.WGRAD_STREAM = side if plan is not None else None
        announced = set()

        def done(tag):          # (backward_train's bucket boundary: slab reduction and the hooks on the weight-gradient stream)
            announced.add(tag)
            if side is not None:
                if hook is not None or final is not None:
                    side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    plan.reduce(tag)
                    if hook is not None:
                        hook(tag)
                if final is not None:
                    final(tag, side)
                return
            if plan is not None:
                plan.reduce(tag)
            if hook is not None:
                hook(tag)

        # every iteration of a run clears the same tensors: their flat ranges, merged, by the library's fill (no stock operator in the step)
        st = self.store
        merged, prev_dead = [], False
        for l, e in zip(self.live_entries(False, True), (e for e in st.entries if e["param"].requires_grad)):
            if not l:
                if prev_dead:          # (what lies between two neighbouring dead tensors is padding: cleared with them)
                    merged[-1][1] = e["offset"] + e["numel"]
                else:
                    merged.append([e["offset"], e["offset"] + e["numel"]])
            prev_dead = not l
        for a, b in merged:
            ops.zero_(st.grads[a:b])
        dweak = wh.group.bwd(c.weak_feat, c.dy_weak, need_dx=True)
        done("heads")
        dpool = c.head.bwd(c.head_ctx, dweak)
        done("weak_box_head" if c.head is rh.weak_box_head else "box_head")
        if self.backbone.first_trainable_stage() < 3:
            g = torch.empty_like(c.feat)
            rh.pool_bwd_gather(ops.as_f32(dpool), c.n_weak, c.feat.shape[1], c.feat.shape[2], c.rois, g, image_offset=0, mask_ref=c.feat,
                               argmax=c.pool_argmax)
            self.backbone.bwd(c.bb_ctx, g, on_stage_done=done)
        for tag in dict.fromkeys(t for t, _, _ in st.tags):
            if tag not in announced:
                done(tag)
        if side is not None:
            if self.overlap_optimizer_tail and not torch.cuda.is_current_stream_capturing():
                side.wait_stream(torch.cuda.current_stream())
                self._tail_pending = side
            else:
                torch.cuda.current_stream().wait_stream(side)
        ops.WGRAD_STREAM = None

    def train_step_only_weak(self, batch, optimizer=None):
        """forward + backward (+ a solver.MaskedFlatSGD update) of the weak-only step without torch.autograd; -> the device loss vector"""
        step = self.forward_train_only_weak(batch)
        if optimizer is not None:
            optimizer.set_live(self.live_entries(False, True))          # before the backward: an early per-bucket update reads it
        self.backward_train_only_weak(step)
        if optimizer is not None:
            optimizer.step()
        return step.losses

    def _streams_on(self):
        """HIP-stream overlap (independent Res5 heads, weight-gradient kernels) -- on by default on the GPU."""
        if not self.overlap_streams or self.device.type != "cuda" or self.plan is None:
            return False   # (without the plan the wgrad kernels share one workspace and must stay on one stream)
        if getattr(self, "_head_stream", None) is None:
            # UNIT_STREAM_MERGE (experiment switch): which of the three side roles share ONE stream object -- "hw" head + weight gradients,
            # "hr" head + RPN branch, "wr" weight gradients + RPN branch, "all" one side stream; "" (default) = three streams placed by a probe
            # on three hardware queues of their own (profiles/r04_exp_stream_queues.txt)
            merge = os.environ.get("UNIT_STREAM_MERGE", "")
            if merge == "" and not torch.cuda.is_current_stream_capturing():
                # (measured, not assumed: ops.streams_on_distinct_queues; under capture the probe cannot run: the streams PyTorch hands out)
                self._head_stream, self._wgrad_stream, self._rpn_stream = ops.streams_on_distinct_queues(self.device, 3)
                return True
            self._head_stream = torch.cuda.Stream(self.device)
            self._wgrad_stream = self._head_stream if merge in ("hw", "all") else torch.cuda.Stream(self.device)
            self._rpn_stream = (self._head_stream if merge in ("hr", "all") else self._wgrad_stream if merge == "wr"
                                else torch.cuda.Stream(self.device))
        return True

    def _reattach_grads(self):
        """optimizer.zero_grad(set_to_none=True) drops .grad: point them at the flat gradient buffer again."""
        st = self.store
        if st is None:
            return
        for e in st.entries:
            p = e["param"]
            if p.requires_grad and p.grad is None:
                p.grad = st._view(st.grads, e["offset"], p)

    @property
    def loss_names(self):
        """the slots of the step's loss vector: LOSS_NAMES, then the weak head's loss_regression_cls / loss_regression_bbox when
        WEAK_DETECTOR.REGRESSION_BRANCH is on (a model without the switch keeps its nine slots)"""
        from .fast_rcnn import REGRESSION_LOSSES
        wh = getattr(getattr(self.roi_heads, "box_predictor", None), "weak_detector_head", None)
        return LOSS_NAMES + (REGRESSION_LOSSES if getattr(wh, "regression_branch", False) else [])

    # ------------------------------------------------------------------ plugin surface
    def forward(self, batched_inputs, weak_batched_inputs=None, return_similarity=False, train_only_weak=False):
        """rcnn.py:433. (Tests that need reproducible sampling set `model.next_perms = {...}` before the call: the explicit-
        permutation contract of the samplers, consumed once.)"""
        perms, self.next_perms = getattr(self, "next_perms", None), None
        if not self.training:
            return self.inference(batched_inputs, return_similarity=return_similarity)
        batch = batched_inputs if isinstance(batched_inputs, PackedBatch) else self.pack_batch(batched_inputs, weak_batched_inputs)
        if train_only_weak:          # rcnn.py:433 with batched_inputs=None (TrainerOnlyWeak, engine/defaults.py:391): the weak-only plan
            step = self.forward_train_only_weak(batch)
            if self._anchor is None or self._anchor.device != self.device:
                self._anchor = torch.zeros(1, device=self.device, requires_grad=True)
            all_names, names = self.loss_names, self.only_weak_loss_names
            used = torch.tensor([n in names for n in all_names], device=self.device)
            lv = _StepFn.apply(self._anchor, self, step, step.losses, used)
            return {n: lv[all_names.index(n)] for n in names}
        step = self.forward_train(batch, perms)
        if self._anchor is None or self._anchor.device != self.device:
            self._anchor = torch.zeros(1, device=self.device, requires_grad=True)
        all_names = self.loss_names
        names = self._returned_losses(batch)
        if step.mask_ctx is None:
            names = [n for n in names if n != "loss_mask"]
        used = torch.tensor([n in names for n in all_names], device=self.device)
        lv = _StepFn.apply(self._anchor, self, step, step.losses, used)
        return {n: lv[all_names.index(n)] for n in names}

    def _returned_losses(self, batch):
        """the keys of the dictionary `forward` returns for this batch (before the mask loss is dropped for a step without masks)"""
        return self.loss_names if batch.n_weak > 0 else [n for n in LOSS_NAMES if not (n.startswith("loss_oicr") or n == "loss_im_cls")]

    def train_step(self, batch, optimizer=None, perms=None):
        """forward + backward (+ optimizer) without going through torch.autograd; returns the device loss vector."""
        step = self.forward_train(batch, perms, early_backward=True)
        self.backward_train(step)
        if optimizer is not None:
            optimizer.step()
        return step.losses

    def inference(self, batched_inputs, detected_instances=None, do_postprocess=True, return_similarity=False):
        from .inference import inference as _inf
        self.join_optimizer_tail()
        return _inf(self, batched_inputs, do_postprocess, detected_instances)          # (read under TEST.AUG.ENABLED only, where it is refused)


ONLY_WEAK_WITH_SUPERVISED = (
    "train_only_weak=True with supervised images is not supported: in the reference only the ROI heads read the flag (roi_heads.py:497, :560 "
    "skip the supervised RoIs) while the RPN still trains on the supervised images (meta_arch/rcnn.py:463-464); the fused plan has no step "
    "with an RPN branch but without supervised RoIs. TrainerOnlyWeak (engine/defaults.py:391) passes batched_inputs=None")
ONLY_WEAK_MASK_HEAD = (
    "train_only_weak=True is not supported with {}: the reference calls _forward_mask(None, None, box_features=None) "
    "(roi_heads.py:813), which has no supervised proposals to select foreground RoIs from")
ONLY_WEAK_FINETUNE = (
    "train_only_weak=True is not supported with {}: its _forward_box calls get_similarity_matrices(None) (roi_heads.py:618) on the "
    "supervised box features the mode does not compute")
ONLY_WEAK_X3 = ("train_only_weak=True: compute_mode \"bf16x3\" has not been taken through a step without supervised images; use \"bf16\" or "
                "\"fp32\"")
ONLY_WEAK_RPN_CLASS = (
    "WeaklySupervisedRCNNRPN does not take train_only_weak: its forward preprocesses batched_inputs unconditionally "
    "(meta_arch/rcnn.py:550) and cannot take None")
ONLY_WEAK_STEP_MODES = (
    "TrainerOnlyWeak runs eagerly only: engine.GraphedStep / ReplayedStep do not take the weak-only step yet (its optimizer update is the "
    "masked kernel, whose mask is not part of a batch key). Use use_graph=False, use_replay=False")

WEAK_RPN_LOSSES = ["weak_loss_rpn_cls", "weak_loss_rpn_loc"]

TRAIN_USING_WEAK_REFUSED = (
    "MODEL.ROI_HEADS.TRAIN_USING_WEAK: True is not supported: the reference's branch (meta_arch/rcnn.py:580-587, :611-620) calls the ROI heads "
    "with return_proposals=True, which this project refuses, and its precomputed-proposal form stops in a debugger (:640-641)")
NOT_AN_RPN = ("WeaklySupervisedRCNNRPN trains the RPN on pseudo ground truth (meta_arch/rcnn.py:570-609): MODEL.PROPOSAL_GENERATOR.NAME "
              "must name an RPN (WSRPN), got '{}'")
STEP_MODES_REFUSED = (
    "WeaklySupervisedRCNNRPN runs eagerly only: engine.GraphedStep / ReplayedStep do not take it yet. Missing: the weak half (a second "
    "backbone pass, the eval-mode ROI heads, unit_pseudo_gt, and the second row group it hands to the RPN head's backward across the "
    "supervised forward plan) has not been taken through a capture or a recording -- its buffers are not part of the static-input and "
    "memory-pool contract of a captured step. Use TrainerNoMeta(use_graph=False, use_replay=False)")


@META_ARCH_REGISTRY.register()
class WeaklySupervisedRCNNRPN(WeaklySupervisedRCNNNoMeta):
    """meta_arch/rcnn.py:544-654: image-level labels train the RPN. The supervised images take the step of WeaklySupervisedRCNNNoMeta
    WITHOUT weak inputs (:644 passes weak_*=None to the ROI heads). The weak images go, without gradient, through the backbone (:558-560, a
    pass of their own, padded to their own largest image), the training-mode RPN (:576) and the eval-mode ROI heads (:577-579); their
    detections of a labelled class above WEAK_RPN_SCORE_TRESHOLD become pseudo ground truth (:594-599, unit_pseudo_gt) and the RPN loss
    against it is added as weak_loss_rpn_cls / weak_loss_rpn_loc (:601-609, :622-624).

    One batched loss launch restates the reference's per-image loop: image i with pseudo ground truth adds
    RPN loss_i / (BATCH_SIZE_PER_IMAGE x 1) x loss_weight x threshold x WEAK_PROPOSAL_DIVISOR (the loc term x 0.0 instead when
    TRAIN_PROPOSAL_REGRESSOR is off), an image without adds 0 (its anchor labels are gated to -1), the result is the mean over the weak
    images: normaliser BATCH_SIZE_PER_IMAGE, weights loss_weight x threshold x divisor / n_weak. The gradient reaches the RPN head's three
    convolutions only, as a second row group of the supervised images' RPN backward (StandardRPNHead.bwd): the gradient-bucket hooks see
    the sum. Same state-dict keys, same inference as WeaklySupervisedRCNNNoMeta."""

    step_modes_refused = STEP_MODES_REFUSED
    only_weak_refused = ONLY_WEAK_RPN_CLASS

    def __init__(self, cfg, thing_classes=None):
        from .inference import UnsupportedConfig
        from .rpn import WSRPN
        if cfg.MODEL.ROI_HEADS.TRAIN_USING_WEAK:
            raise UnsupportedConfig(TRAIN_USING_WEAK_REFUSED)
        name = cfg.MODEL.PROPOSAL_GENERATOR.NAME
        if name not in PROPOSAL_GENERATOR_REGISTRY or not issubclass(PROPOSAL_GENERATOR_REGISTRY.get(name), WSRPN):
            raise UnsupportedConfig(NOT_AN_RPN.format(name))
        super().__init__(cfg, thing_classes)
        self.weak_rpn_score_threshold = float(cfg.MODEL.PROPOSAL_GENERATOR.WEAK_RPN_SCORE_TRESHOLD)
        self.train_proposal_regressor = bool(cfg.MODEL.ROI_HEADS.TRAIN_PROPOSAL_REGRESSOR)
        self.weak_proposal_divisor = float(cfg.MODEL.ROI_HEADS.WEAK_PROPOSAL_DIVISOR)
        if int(cfg.TEST.DETECTIONS_PER_IMAGE) > 256:
            raise UnsupportedConfig("WeaklySupervisedRCNNRPN: TEST.DETECTIONS_PER_IMAGE > 256 -- the detections of a weak image are its candidate "
                                    "ground-truth boxes and the anchor matcher (unit_iou_match) holds at most 256 per image")

    @property
    def loss_names(self):
        """the base class's slots, then weak_loss_rpn_cls / weak_loss_rpn_loc"""
        return super().loss_names + WEAK_RPN_LOSSES

    def _returned_losses(self, batch):
        # rcnn.py:644: the ROI heads never see the weak batch -> no loss_im_cls / loss_oicr_* (nor the weak head's regression losses);
        # :630-632: without weak inputs no weak keys
        names = [n for n in LOSS_NAMES if not (n.startswith("loss_oicr") or n == "loss_im_cls")]
        return names + (WEAK_RPN_LOSSES if batch.n_weak > 0 else [])

    def _clear_unproduced(self, c):
        # No step of this class produces a gradient for the weak heads (rcnn.py:644 keeps the weak batch from the ROI heads). Their ranges of
        # the flat gradient buffer are zero from its allocation and nothing ever writes them: cleared once per buffer, not once per step
        if self.__dict__.get("_cleared_store") is not self.store:
            super()._clear_unproduced(c)
            self._cleared_store = self.store

    def weak_permutations(self, n_weak, n_anchor):
        """one anchor-sampling permutation per weak image (`weak_rpn` of the explicit-permutation contract), drawn on the device from the
        same (seed, step counter) as the step's other draws under a stream id of its own"""
        seed, counter = self._rng()
        return ops.random_permutations(n_weak, n_anchor, seed, counter, 2, self.device)

    def forward_train(self, batch, perms=None, early_backward=False, proposals=None):
        """-> the base class's step context of the SUPERVISED images (rcnn.py:644), its loss vector two slots longer; `c.weak` holds the weak
        half's device tensors (pseudo ground truth, kept detection indices, anchor labels), None without weak images"""
        rpn = self.proposal_generator
        rpn.rpn_head.second_group = None
        self.__dict__.pop("_step_losses", None)
        n_sup, n_weak = batch.n_sup, batch.n_weak
        if n_sup == 0:
            raise ValueError("WeaklySupervisedRCNNRPN.forward needs supervised images (rcnn.py:550 preprocesses batched_inputs unconditionally)")
        if proposals is not None:
            raise NotImplementedError("WeaklySupervisedRCNNRPN: precomputed proposals -- the reference's branch (rcnn.py:633-642) has no weak RPN loss")
        sup_batch = PackedBatch(batch.images[:n_sup], batch.gt_boxes, batch.gt_classes, batch.gt_count, n_sup, None, batch.gt_masks)
        if n_weak == 0:
            c = super().forward_train(sup_batch, perms, early_backward)
            c.weak = None
            return c
        if self._x3:
            raise NotImplementedError("WeaklySupervisedRCNNRPN: compute_mode \"bf16x3\" is not wired through the two-group RPN backward; use \"bf16\" or \"fp32\"")
        self._ensure_ready()
        self.join_optimizer_tail()          # the weak pass reads every weight now: no optimizer tail beside it
        dt = self.compute_dtype
        from .inference import roi_heads_inference
        losses = ops.zeros(len(self.loss_names), torch.float32, self.device)
        # ---- weak half (rcnn.py:557-609), nothing of it saved for a backward but the RPN head's two activations
        xw, sizes_w = ops.preprocess_images(batch.images[n_sup:], self._pixel_mean, self._pixel_std, dt, 8, self.normalize_images)
        feat_w, _ = self.backbone.fwd(xw)
        head_w, rpn_ctx_w = rpn.rpn_head.fwd(feat_w, save=True)
        anchors_w = rpn.anchor_generator.grid(feat_w.shape[1], feat_w.shape[2])
        hw_w = self._sizes_on_device(sizes_w)
        props, _, pcount = rpn.predict_proposals(head_w, anchors_w, hw_w, True)          # training-mode top-k: only roi_heads is in eval (:577)
        boxes, scores, classes, _, count, _ = roi_heads_inference(self.roi_heads, feat_w, props, pcount, hw_w, dt, with_mask=False)
        gt_boxes, gt_count, kept = ops.pseudo_gt(boxes, scores, classes, count, batch.multihot, self.weak_rpn_score_threshold)
        wperm = perms.get("weak_rpn") if perms is not None else None
        if wperm is None:
            wperm = self.weak_permutations(n_weak, anchors_w.shape[0])
        labels_w, match_w, _ = rpn.label_and_sample_anchors(anchors_w, gt_boxes, gt_count, wperm)
        ops.gate_anchor_labels(labels_w, gt_count)          # an image without pseudo ground truth adds 0 (:607-609)
        f = self.weak_rpn_score_threshold * self.weak_proposal_divisor / n_weak
        w_loc = rpn.loss_weight["loss_rpn_loc"] * f if self.train_proposal_regressor else 0.0          # (:606: x 0.0)
        _, dhead_w = ops.rpn_loss(head_w, rpn.num_anchors, rpn.num_anchors, labels_w, match_w, gt_boxes, anchors_w, rpn.batch_size_per_image, dt,
                                  loss_out=losses[len(losses) - 2:], weights=(rpn.loss_weight["loss_rpn_cls"] * f, w_loc),
                                  loss_type=rpn.box_reg_loss_type, beta=rpn.smooth_l1_beta)
        if any(p.requires_grad for p in rpn.rpn_head.parameters()):
            group = (rpn_ctx_w[0], rpn_ctx_w[1], dhead_w)
            if self._streams_on():          # the RPN backward may run on the RPN-branch stream, its weight gradients on theirs
                for t in group + (losses,):
                    t.record_stream(self._rpn_stream)
                    t.record_stream(self._wgrad_stream)
            rpn.rpn_head.second_group = group          # consumed by the step's one RPN-head backward
        self._step_losses = losses
        c = super().forward_train(sup_batch, perms, early_backward)
        c.weak = dict(gt_boxes=gt_boxes, gt_count=gt_count, kept=kept, anchor_labels=labels_w, det_count=count, det_scores=scores, det_classes=classes)
        return c


def build_model(cfg, thing_classes=None):
    """detectron2.modeling.build_model: META_ARCH_REGISTRY lookup + .to(cfg.MODEL.DEVICE)."""
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg, thing_classes)
    model.to(torch.device(cfg.MODEL.DEVICE))
    return model
