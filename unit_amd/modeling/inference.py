"""Eval / inference path -- /root/reference/modeling/meta_arch/rcnn.py:493-542 (non-TTA branch :527-538),
WSROIHeadNoMeta.forward eval branch (roi_heads.py:585-591 -> _forward_box :519-551), predictor eval transfer
(fast_rcnn.py:401-423), `inference` (:455-468 -> detectron2 fast_rcnn_inference) and `_postprocess` (rcnn.py:411-429).
Everything stays on the device; only the final per-image detection count is read back to build the `Instances` lists.
Under TEST.AUG.ENABLED the TTA branch (rcnn.py:495-527 over the views of _init_tta_fn, :209-248): `inference_tta` below."""
import torch

from .. import ops
from ..structures import Boxes, Instances


class UnsupportedConfig(ValueError, AssertionError):
    """a configuration this project refuses. A ValueError, as a bad value of a config key is; also an AssertionError, which is what every other
    refusal at construction of the predictors raises (`assert ...` in modeling/fast_rcnn.py) and what callers of build_model therefore catch"""


VISUAL_WITH_REGRESSION_BRANCH = (
    "a \"visual\" term in MODEL.ROI_HEADS.FINETUNE_TERMS together with WEAK_DETECTOR.REGRESSION_BRANCH is not supported: the reference's "
    "get_similarity_matrices reads evaluation(...)[0][0] as a list of refinement streams (roi_heads.py:250-252), which under the switch is one "
    "[R, K+1] tensor whose mean's index_select(1, ...) fails. Use [\"lingual\"] or [] for every head")


def _rh(m):
    return getattr(m, "roi_heads", m)


def class_roles(model):
    """device-side index tables for the base->novel transfer (built once per device). `model`: the meta-architecture or its ROI heads."""
    rh = _rh(model)
    cache = getattr(rh, "_role_cache", None)
    dev = next(rh.parameters()).device
    if cache is not None and cache["dev"] == dev:
        return cache
    k = rh.num_classes
    base, novel = list(rh._base_classes), list(rh._novel_classes)
    role = torch.zeros(k, dtype=torch.int8)
    slot = torch.zeros(k, dtype=torch.int32)
    for i, c in enumerate(base):
        role[c], slot[c] = 1, i
    for i, c in enumerate(novel):
        role[c], slot[c] = 2, i
    idx = torch.tensor(rh._coco_indexer, dtype=torch.int32)
    cache = dict(dev=dev, base=torch.tensor(base, dtype=torch.int32, device=dev), novel=torch.tensor(novel, dtype=torch.int32, device=dev),
                 role=role.to(dev), slot=slot.to(dev),
                 emb_novel=idx[novel].to(dev).contiguous(), emb_base=idx[base].to(dev).contiguous())
    rh._role_cache = cache
    return cache


def similarity_dict(model, lin_weak_on_box, want_ctx=False):
    """WSROIHead.get_similarity_matrices roi_heads.py:245-336 -> {head: [R,n,b]}. Every head's term list goes by its plan
    (similarity_terms.parse_terms): 'lingual' / 'visual' alone under "Sum" take unit_similarity as ever, every other plan the static part
    (unit_similarity_static) and unit_similarity_ex.
    (want_ctx: also the lingual matrix and, for the backward, {head: (plan, static part or None)})"""
    rh = _rh(model)
    bp = rh.box_predictor
    plans = rh.term_plans()          # (parsed at construction; re-parsed, and refused if need be, when the lists were edited on the built model)
    t = class_roles(rh)
    wh = bp.weak_detector_head
    lingual = ops.embedding_similarity(bp.embeddings.weight, t["emb_novel"], t["emb_base"])       # fast_rcnn.py:376-382
    oicr = (wh.col_oicr[0], wh.oicr_iter, rh.num_classes + 1)
    sims, statics, out, ctx = {}, {}, {}, {}
    for head, plan in plans.items():
        static = None
        if not plan.plain:
            sk = "constant" if plan.constant else plan.static_key
            if sk not in statics:          # Average / None / "Product" never read the static part: any [n, b] buffer stands in, no launch
                statics[sk] = lingual if plan.constant else ops.similarity_static(wh.group.w32, *oicr, t["base"], t["novel"], lingual, plan)
            static = statics[sk]
        if plan not in sims:
            if plan.plain:
                sims[plan] = ops.similarity(lin_weak_on_box, *oicr, t["base"], lingual, t["novel"].numel(), rh.visual_threshold, *plan.key)
            else:
                sims[plan] = ops.similarity_ex(lin_weak_on_box, *oicr, t["base"], static, rh.visual_threshold, plan)
        out[head] = sims[plan]
        ctx[head] = (plan, static)
    if want_ctx:
        return out, lingual, ctx
    return out


def similarity_backward(rh, lin_weak_on_box, lingual, ctx, dsim, grad_dtype):
    """d(loss)/d(similarity matrix) -> d(loss)/d(the weak head's logits on the box features), by the plan that `similarity_dict(..., want_ctx=True)`
    returned (rcnn.backward_train and train_modules._HeadsFn.backward: the two sites where the box head trains under the fine-tune heads)"""
    assert len(set(p for p, _ in ctx.values())) == 1, "fine-tune backward: one similarity matrix for all heads (equal FINETUNE_TERMS)"
    plan, static = next(iter(ctx.values()))
    t = class_roles(rh)
    wh = rh.box_predictor.weak_detector_head
    oicr = (wh.col_oicr[0], wh.oicr_iter, rh.num_classes + 1)
    if plan.plain:
        return ops.similarity_bwd(lin_weak_on_box, *oicr, t["base"], lingual, t["novel"].numel(), rh.visual_threshold, *plan.key, dsim, grad_dtype)
    return ops.similarity_bwd_ex(lin_weak_on_box, *oicr, t["base"], static, rh.visual_threshold, plan, dsim, grad_dtype)


def similarity_matrices(model, lin_weak_on_box):
    d = similarity_dict(model, lin_weak_on_box)
    return d["cls"], d["bbox"]


def roi_heads_predict(rh, feat, props, pcount):
    """the "predict" half of the eval branch: _forward_box (roi_heads.py:519-551) up to the predictor's eval transfer (fast_rcnn.py:401-423)
    -> (scores [N*Rcap, K+1], bbox [N*Rcap, 4K], similarity dict). What the reference's predictors return under tta=True before the softmax
    (fast_rcnn.py:456-458); the single-scale path and every TTA view run exactly this."""
    bp = rh.box_predictor
    wh = bp.weak_detector_head
    rcap = props.shape[1]
    rois5, _ = ops.first_k_rois(props, pcount, rcap, 0)
    pooled = rh.pool(feat, rois5)
    box_feat, _ = rh.box_head.fwd(pooled)
    sup_weak = rh.weak_box_head.fwd(pooled)[0] if rh.weak_box_head is not None else box_feat
    lin_sup = bp.group.fwd(box_feat)
    lin_w_box = wh.group.fwd(box_feat)                       # visual similarity uses box_head features (roi_heads.py:250-252)
    lin_w_sup = wh.group.fwd(sup_weak) if rh.weak_box_head is not None else lin_w_box
    sims = similarity_dict(rh, lin_w_box)
    t = class_roles(rh)
    ft = bp.group_ft.fwd(box_feat) if getattr(bp, "finetune", False) else None
    # REGRESSION_BRANCH: + the weak deltas after the transfer (fast_rcnn.py:414-426) -- Base: a second launch; FineTune: inside the one launch
    scores, bbox = bp.transfer(lin_sup, lin_w_sup, sims["cls"], sims["bbox"], t, ft=ft)
    return scores, bbox, sims


def roi_heads_detect(rh, feat, probs, bbox, props, pcount, hw, sims, with_mask=True, want_similarity=False, cand_cap=None, nms=None):
    """the "detect" half: `inference` (fast_rcnn.py:455-468, fast_rcnn_inference) on class probabilities [N*Rcap, K+1] and deltas [N*Rcap, 4K]
    -> forward_with_given_boxes (mask, roi_heads.py:776-781). Outputs as roi_heads_inference. cand_cap / nms: as ops.detections."""
    bp = rh.box_predictor
    n = props.shape[0]
    rcap = props.shape[1]
    boxes, sc, cls, roi, cnt = ops.detections(probs, bbox, props, pcount, hw, bp.bbox_reg_weights, bp.test_score_thresh,
                                              bp.test_nms_thresh, bp.test_topk_per_image, cand_cap=cand_cap, nms=nms)
    # a16 eval: forward_with_given_boxes (roi_heads.py:776-781) -> mask head on the detected boxes (before postprocess)
    mask_probs = None
    mh = getattr(rh, "mask_head", None)
    sim_seg = None
    if mh is not None and "seg" in rh.terms and (with_mask or want_similarity):
        sim_seg = ops.gather_rows(sims["seg"], roi, rcap)          # similarity['seg'][filter_inds] (roi_heads.py:768-771)
    if mh is not None and with_mask:
        topk = boxes.shape[1]
        det_rois = ops.boxes_to_rois5(boxes)
        mask_probs = mask_probs_on_boxes(rh, feat, det_rois, cls.view(-1).contiguous(), sim_seg).view(n, topk, mh.mask_size, mh.mask_size)
    if want_similarity:
        return boxes, sc, cls, roi, cnt, mask_probs, sim_seg
    return boxes, sc, cls, roi, cnt, mask_probs


def roi_heads_inference(rh, feat, props, pcount, hw, dt, with_mask=True, want_similarity=False):
    """eval branch of WSROIHead*.forward (roi_heads.py:585-591 / :796-801): _forward_box (:519-551) -> predictor eval transfer
    (fast_rcnn.py:401-423) -> `inference` (:455-468, fast_rcnn_inference) -> forward_with_given_boxes (mask, :776-781).
    feat NHWC [N,H,W,C] (compute dtype), props [N,P,4], pcount int32 [N], hw fp32 [N,2] (device)
    -> boxes [N,topk,4], scores, classes, roi index, count [N], mask probabilities [N,topk,14,14] or None
    with_mask=False: the box half only (the reference's `_forward_box`); want_similarity: additionally the rows of the 'seg' similarity
    matrix of the detections, [N*topk, ...] (similarity['seg'][filter_inds], roi_heads.py:768-771), or None without a 'seg' term"""
    scores, bbox, sims = roi_heads_predict(rh, feat, props, pcount)
    probs = ops.softmax_rows(scores, rh.num_classes + 1)
    return roi_heads_detect(rh, feat, probs, bbox, props, pcount, hw, sims, with_mask, want_similarity)


def mask_probs_on_boxes(rh, feat, rois5, classes, sim_seg):
    """forward_with_given_boxes / _forward_mask eval (roi_heads.py:691-710, :776-781): box pooler + box head on the GIVEN boxes, mask
    head on the res5 maps, probability of each box's class (base->novel transfer through sim_seg rows). -> [R, 14, 14]"""
    _, dctx = rh.box_head.fwd(rh.pool(feat, rois5), keep_map=True)
    return rh.mask_head.probs(dctx[1], classes, sim_seg, class_roles(rh))


# ---------------------------------------------------------------------------------------------------------------------------------------
# Test-time augmentation (TEST.AUG): the TTA branch of WeaklySupervisedRCNNNoMeta.inference / WeaklySupervisedRCNNRPN.inference,
# meta_arch/rcnn.py:495-527 and :658-690, over the views of _init_tta_fn (:209-248). On precomputed proposals only.
TTA_NEEDS_PROPOSALS = (
    "TEST.AUG.ENABLED needs precomputed proposals: an input without \"proposals\" was given. The reference reads x[\"proposals\"] when it combines "
    "the views (meta_arch/rcnn.py:515) and when it builds them (:226); its RPN-per-view form would stack the predictions of unrelated proposal rows "
    "(:516, :524)")
TTA_DETECTED_INSTANCES = "TEST.AUG.ENABLED with detected_instances is not implemented, as in the reference (meta_arch/rcnn.py:513-514)"
TTA_MASK_HEADS = (
    "TEST.AUG.ENABLED on a model with a mask head is not supported: the reference's own TTA cannot run there. Under tta=True its predictors return "
    "[scores, deltas] (fast_rcnn.py:457-458) and WSROIHeadNoMetaWithMask / WSROIHeadWithMaskFineTune._forward_box then stop at `assert "
    "len(pred_instances) == 1` (roi_heads.py:770, :882), the similarity dictionary never being None in eval mode: there is no result to follow")
TTA_NO_SIZES = "TEST.AUG.ENABLED with an empty TEST.AUG.MIN_SIZES: there is no view to run (the reference would stack an empty list, meta_arch/rcnn.py:516)"
TTA_TOO_MANY_CANDIDATES = (
    "TEST.AUG.ENABLED: {r} proposals x {k} classes = {c} detection candidates exceed the {limit} the NMS kernel takes per image. Summed over the "
    "views almost every (RoI, class) score passes SCORE_THRESH_TEST, so the TTA path sizes the candidate list to all of them and refuses instead of "
    "cutting the list: give at most {rmax} proposals")


def tta_view_plan(h, w, aug):
    """the views of an (h, w) image, in the reference's order (_init_tta_fn, meta_arch/rcnn.py:221-246): for every s of TEST.AUG.MIN_SIZES the
    ResizeShortestEdge(s, MAX_SIZE) size, directly followed by its flipped twin under FLIP -> [(new_h, new_w, flip)...]"""
    from ..data_pipeline import resize_shortest_edge_size
    plan = []
    for s in aug.MIN_SIZES:
        nh, nw = resize_shortest_edge_size(int(h), int(w), int(s), int(aug.MAX_SIZE))
        plan.append((nh, nw, False))
        if aug.FLIP:
            plan.append((nh, nw, True))
    return plan


def _proposal_boxes(p):
    return (p.proposal_boxes.tensor if hasattr(p.proposal_boxes, "tensor") else p.proposal_boxes).float()


def tta_check(aug, batched_inputs, num_classes, detected_instances=None, candidate_limit=None, mask_on=False):
    """the refusals of a TTA call, before anything runs (host only). candidate_limit: ops.max_detection_candidates(), read out of the NMS kernel"""
    if detected_instances is not None:
        raise NotImplementedError(TTA_DETECTED_INSTANCES)
    if mask_on:
        raise UnsupportedConfig(TTA_MASK_HEADS)
    if len(aug.MIN_SIZES) == 0:
        raise UnsupportedConfig(TTA_NO_SIZES)
    for x in batched_inputs:
        if "proposals" not in x:
            raise UnsupportedConfig(TTA_NEEDS_PROPOSALS)
    limit = ops.max_detection_candidates() if candidate_limit is None else int(candidate_limit)
    for x in batched_inputs:
        r = max(len(_proposal_boxes(x["proposals"])), 1)
        if r * num_classes > limit:
            raise UnsupportedConfig(TTA_TOO_MANY_CANDIDATES.format(r=r, k=num_classes, c=r * num_classes, limit=limit, rmax=limit // num_classes))


def _tta_pipeline(model):
    from ..data_pipeline import DeviceInputPipeline
    key = (model.compute_dtype, model.device, bool(model.normalize_images))
    pipe = model.__dict__.get("_tta_pipe")
    if pipe is None or pipe[0] != key:          # (the coefficient tables are cached per size pair inside)
        pipe = (key, DeviceInputPipeline(model._pixel_mean, model._pixel_std, dtype=model.compute_dtype, cpad=8,
                                         normalize_images=model.normalize_images, device=model.device))
        model.__dict__["_tta_pipe"] = pipe
    return pipe[1]


def tta_predict(model, x, twin_batch=True, want_views=False):
    """one input through every view -> (probs_sum [Rcap, K+1], delta_mean [Rcap, 4K], props [1, Rcap, 4], count int32 [1], image_size).
    Per size the uint8 image is resized once (no pass when the size is unchanged); under FLIP unit_preprocess_u8 writes it with hflip 0 and 1
    into a batch of two, which makes ONE backbone + ROI-heads pass (twin_batch=False: two passes of one image, the form it is measured
    against). The RPN head does not run. No host sync. want_views: additionally [(resized uint8 image, the views' boxes)...] per size."""
    from .. import data_pipeline as dpl
    from .._lib import check, lib
    rh, dev, dt = model.roi_heads, model.device, model.compute_dtype
    aug = model.cfg.TEST.AUG
    k = rh.num_classes
    img = x["image"].to(dev)
    u8 = ops.image_chw_to_u8(img if img.dtype == torch.uint8 else img.float())          # image.astype(np.uint8), rcnn.py:218
    h, w = int(u8.shape[0]), int(u8.shape[1])
    plan = tta_view_plan(h, w, aug)
    n_views = len(plan)
    n_in = 2 if aug.FLIP else 1
    boxes = _proposal_boxes(x["proposals"]).to(dev).contiguous()
    p = boxes.shape[0]
    rcap = max(p, 1)
    count = model._const_on_device(("tta_count", p), lambda: torch.tensor([p, p], dtype=torch.int32))
    table = model._const_on_device(("tta_views", h, w, tuple(plan)), lambda: ops.tta_view_table(h, w, plan))
    vboxes = ops.tta_boxes(boxes, count, table, rcap)          # [V, Rcap, 4]: rcnn.py:226, :240
    probs_sum = torch.empty((rcap, k + 1), dtype=torch.float32, device=dev)
    delta_sum = torch.empty((rcap, 4 * k), dtype=torch.float32, device=dev)
    delta_mean = torch.empty((rcap, 4 * k), dtype=torch.float32, device=dev)
    pipe = _tta_pipeline(model)
    views = []
    for i in range(n_views // n_in):
        nh, nw, _ = plan[i * n_in]
        r8 = pipe.resize(u8, nh, nw)
        batch = torch.empty((n_in, nh, nw, pipe.cpad), dtype=dt, device=dev)
        for j in range(n_in):
            check(lib().unit_preprocess_u8(ops._p(r8), r8.shape[2], nh, nw, j, pipe.mean, pipe.std, pipe.prescale, ops._p(batch[j]), ops.dt(dt),
                                           nh, nw, pipe.cpad, ops._s()), "preprocess_u8")
        vb = vboxes[i * n_in:(i + 1) * n_in]
        if want_views:
            views.append((r8, vb))
        if twin_batch or n_in == 1:
            feat, _ = model.backbone.fwd(batch)
            scores, bbox, _ = roi_heads_predict(rh, feat, vb, count[:n_in])
            ops.tta_accumulate(scores, bbox, k, rcap, i * n_in, n_views, probs_sum, delta_sum, delta_mean, count, n_in, view_rows=rcap)
        else:
            for j in range(n_in):
                feat, _ = model.backbone.fwd(batch[j:j + 1])
                scores, bbox, _ = roi_heads_predict(rh, feat, vb[j:j + 1], count[:1])
                ops.tta_accumulate(scores, bbox, k, rcap, i * n_in + j, n_views, probs_sum, delta_sum, delta_mean, count, 1)
    image_size = tuple(int(v) for v in getattr(x["proposals"], "image_size", (h, w)))
    out = (probs_sum, delta_mean, boxes.view(1, p, 4) if p else ops.zeros((1, 1, 4), torch.float32, dev), count[:1], image_size)
    return out + (views, plan) if want_views else out


def tta_candidate_limit(num_classes):
    """the candidates a TTA call may have per image: the class-segmented NMS stage's ceiling (ops.max_segmented_candidates(), the sorter's), and
    no class above what one unit_nms problem takes (every proposal is a candidate of every class)"""
    return min(ops.max_segmented_candidates(), ops.max_detection_candidates() * num_classes)


def inference_tta(model, batched_inputs, do_postprocess=True, detected_instances=None, twin_batch=True, nms=None):
    """meta_arch/rcnn.py:495-527: per input, every view through backbone and ROI heads up to the predictor's [scores, deltas]; the class
    probabilities summed (not renormalised: scores up to n_views), the deltas averaged (the flipped views' dx as they are, :524), decoded once
    against the ORIGINAL proposals and their image_size, then fast_rcnn_inference and _postprocess. The branch never reaches
    forward_with_given_boxes, and on the mask ROI heads the reference does not get that far (TTA_MASK_HEADS). More than one input: the per-image procedure in a loop (the reference
    asserts len == 1, :494). nms: the form of the NMS stage (ops.detections); by default the full form up to 65 536 candidates and the
    class-segmented one above."""
    rh = model.roi_heads
    k = rh.num_classes
    tta_check(model.cfg.TEST.AUG, batched_inputs, k, detected_instances, candidate_limit=tta_candidate_limit(k),
              mask_on=getattr(rh, "mask_head", None) is not None)
    results = []
    for x in batched_inputs:
        probs_sum, delta_mean, props, count, image_size = tta_predict(model, x, twin_batch)
        hw = model._sizes_on_device([image_size])
        boxes, sc, cls, roi, cnt, _ = roi_heads_detect(rh, None, probs_sum, delta_mean, props, count, hw, None, with_mask=False,
                                                       cand_cap=props.shape[1] * k, nms=nms)
        # _postprocess (:539-540) is handed the LAST view's image sizes, read only where an input carries no "height" / "width"
        out_hw = None
        if do_postprocess:
            last = tta_view_plan(int(x["image"].shape[-2]), int(x["image"].shape[-1]), model.cfg.TEST.AUG)[-1]
            out_hw = [(x.get("height", last[0]), x.get("width", last[1]))]
        results += build_instances(boxes, sc, cls, roi, cnt, None, [image_size], out_hw, consts=model._const_on_device)
    return results


@torch.no_grad()
def inference(model, batched_inputs, do_postprocess=True, detected_instances=None):
    model._ensure_ready()
    if model.cfg.TEST.AUG.ENABLED:
        return inference_tta(model, batched_inputs, do_postprocess, detected_instances)
    rpn, rh = model.proposal_generator, model.roi_heads
    dt = model.compute_dtype
    dev = model.device
    imgs = [x["image"].to(dev).float() for x in batched_inputs]
    x, sizes = ops.preprocess_images(imgs, model._pixel_mean, model._pixel_std, dt, 8, model.normalize_images)
    feat, _ = model.backbone.fwd(x)
    n, fh, fw, _ = feat.shape
    anchors = rpn.anchor_generator.grid(fh, fw)
    head, _ = rpn.rpn_head.fwd(feat)
    hw = model._sizes_on_device(sizes)          # (uploaded once per distinct value)
    if rpn is not None and "proposals" not in batched_inputs[0]:
        props, pscores, pcount = rpn.predict_proposals(head, anchors, hw, False)
    else:       # precomputed proposals (rcnn.py:533-536)
        props, pcount = pack_proposal_instances([x["proposals"] for x in batched_inputs], dev)
    boxes, sc, cls, roi, cnt, mask_probs = roi_heads_inference(rh, feat, props, pcount, hw, dt)
    out_hw = [(x.get("height", s[0]), x.get("width", s[1])) for x, s in zip(batched_inputs, sizes)]
    return build_instances(boxes, sc, cls, roi, cnt, mask_probs, sizes, out_hw if do_postprocess else None, consts=model._const_on_device)


def pack_proposal_instances(proposals, dev):
    """list[Instances(proposal_boxes)] -> (props [N,P,4] fp32, count int32 [N]) on the device"""
    bs = [(p.proposal_boxes.tensor if hasattr(p.proposal_boxes, "tensor") else p.proposal_boxes).float() for p in proposals]
    cap = max(max(len(b) for b in bs), 1)
    props = torch.zeros((len(bs), cap, 4), dtype=torch.float32, device=dev)
    for i, b in enumerate(bs):
        props[i, : len(b)] = b.to(dev)
    return props, torch.tensor([len(b) for b in bs], dtype=torch.int32).to(dev)


def build_instances(boxes, sc, cls, roi, cnt, mask_probs, sizes, out_hw=None, consts=None):
    """device detections -> the reference's output format: list of {"instances": Instances} after `_postprocess` (rcnn.py:411-429)
    when out_hw is given, else list of Instances in network-input coordinates (what ROI heads return)."""
    dev = boxes.device
    do_postprocess = out_hw is not None
    if do_postprocess:
        mk_scale = lambda: torch.tensor([[o[1] / s[1], o[0] / s[0]] for o, s in zip(out_hw, sizes)], dtype=torch.float32)
        mk_ohw = lambda: torch.tensor(out_hw, dtype=torch.float32)
        if consts is not None:          # GeneralizedRCNN._const_on_device: one upload per distinct value, none in the steady state
            scale, ohw = consts(("pp_scale", tuple(out_hw), tuple(sizes)), mk_scale), consts(("pp_ohw", tuple(out_hw)), mk_ohw)
        else:
            scale, ohw = mk_scale().to(dev), mk_ohw().to(dev)
        nonempty = ops.detector_postprocess(boxes, cnt, scale, ohw)
    # kept rows of every image to the front of its block in ONE launch (the reference indexes every field with a boolean mask per image);
    # after that the per-image fields are views
    boxes, sc, cls64, roi, mask_probs, kept = ops.compact_detections(boxes, sc, cls, roi, cnt, nonempty if do_postprocess else None, mask_probs)
    results = []
    counts = kept.tolist()          # API boundary: python lists of Instances need the counts on the host (the call's one sync)
    for i, c in enumerate(counts):
        size = out_hw[i] if do_postprocess else sizes[i]
        inst = Instances(size, pred_boxes=Boxes(boxes[i, :c]), scores=sc[i, :c], pred_classes=cls64[i, :c])
        inst._roi_index = roi[i, :c]
        if mask_probs is not None:
            mp = mask_probs[i, :c]
            if do_postprocess:
                # detector_postprocess (rcnn.py:423): paste the 14x14 masks into the output image, threshold 0.5 -> bool [R,H,W]
                inst.pred_mask_probs = mp[:, None]
                inst.pred_masks = ops.paste_masks(mp, inst.pred_boxes.tensor, size, 0.5).view(torch.bool)          # (0 / 1 bytes: a view)
            else:
                inst.pred_masks = mp[:, None]                       # (R,1,14,14) like mask_rcnn_inference
        results.append({"instances": inst} if do_postprocess else inst)
    return results
