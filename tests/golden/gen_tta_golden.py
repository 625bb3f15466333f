"""Generates tests/golden/tta_golden.npz by RUNNING THE REFERENCE'S OWN WeaklySupervisedRCNNNoMeta.inference with TEST.AUG on
(/root/reference/modeling/meta_arch/rcnn.py:493-542 over the views of _init_tta_fn, :209-248) in the authoring container, through the machinery
of gen_unit_golden.py / gen_ref_step.py: the reference's meta-architecture, ROI heads and predictors, the un-vendored Detectron2 blocks from the
CPU oracle. After construction the model gets what Detectron2 builds for precomputed proposals and a TTA configuration:
ref.proposal_generator = None, ref.test_augmentations, ref.tta = ref._init_tta_fn(...).

The Detectron2 transforms the reference calls -- T.ResizeShortestEdge, T.RandomFlip, T.AugmentationList, T.AugInput and their apply_box -- are
absent from the image like the rest of Detectron2: the stand-ins below are written from the published v0.3 API (detectron2/data/transforms,
fvcore/transforms/transform.py) with Pillow for the resize, and installed onto the stub `detectron2.data.transforms` module.

Only arrays are committed. Per case: the proposals, each view's (h, w, flip) and transformed boxes, probs_sum, delta_mean, the final boxes /
scores / classes; for the "tta" case also the resized uint8 views. The margins of the decisions (tests/tta_ref.py) are asserted here and
re-asserted by tests/test_tta_cpu.py.      Run here:  python tests/golden/gen_tta_golden.py
"""
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p_ in (HERE, ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import gen_unit_golden as G  # noqa: E402  (installs the stubs, loads the reference's modeling modules)
import gen_ref_step as S  # noqa: E402
import tta_ref  # noqa: E402

d2, orc = G.d2, G.orc
OUT = os.path.join(HERE, "tta_golden.npz")
SEEDS = {"tta": 81, "tta_ft": 302, "tta_mask": 13, "tta_noflip": 14}          # (the first of 11, 21, ... / 12, 22, ... that gives the margins)


# ================================================================================================ detectron2.data.transforms, v0.3
class Transform:
    """fvcore.transforms.transform.Transform: apply_box through the four corners and their min / max"""

    def apply_box(self, box):
        idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
        coords = np.asarray(box).reshape(-1, 4)[:, idxs].reshape(-1, 2)
        coords = self.apply_coords(coords).reshape((-1, 4, 2))
        minxy = coords.min(axis=1)
        maxxy = coords.max(axis=1)
        return np.concatenate((minxy, maxxy), axis=1)


class ResizeTransform(Transform):
    """detectron2.data.transforms.ResizeTransform: PIL resize of a uint8 image, coordinates scaled by new / old"""

    def __init__(self, h, w, new_h, new_w, interp=Image.BILINEAR):
        self.h, self.w, self.new_h, self.new_w, self.interp = h, w, new_h, new_w, interp

    def apply_image(self, img):
        assert img.shape[:2] == (self.h, self.w) and img.dtype == np.uint8
        return np.asarray(Image.fromarray(img).resize((self.new_w, self.new_h), self.interp))

    def apply_coords(self, coords):
        coords[:, 0] = coords[:, 0] * (self.new_w * 1.0 / self.w)
        coords[:, 1] = coords[:, 1] * (self.new_h * 1.0 / self.h)
        return coords


class HFlipTransform(Transform):
    def __init__(self, width):
        self.width = width

    def apply_image(self, img):
        return np.flip(img, axis=1)

    def apply_coords(self, coords):
        coords[:, 0] = self.width - coords[:, 0]
        return coords


class TransformList(Transform):
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def apply_image(self, img):
        for t in self.transforms:
            img = t.apply_image(img)
        return img

    def apply_box(self, box):
        for t in self.transforms:
            box = t.apply_box(box)
        return box


class ResizeShortestEdge:
    def __init__(self, short_edge_length, max_size=sys.maxsize, sample_style="range", interp=Image.BILINEAR):
        assert sample_style == "choice"
        if isinstance(short_edge_length, int):
            short_edge_length = (short_edge_length, short_edge_length)
        self.short_edge_length, self.max_size, self.interp = short_edge_length, max_size, interp

    def get_transform(self, image):
        h, w = image.shape[:2]
        size = np.random.choice(self.short_edge_length)
        scale = size * 1.0 / min(h, w)
        if h < w:
            newh, neww = size, scale * w
        else:
            newh, neww = scale * h, size
        if max(newh, neww) > self.max_size:
            scale = self.max_size * 1.0 / max(newh, neww)
            newh = newh * scale
            neww = neww * scale
        neww = int(neww + 0.5)
        newh = int(newh + 0.5)
        return ResizeTransform(h, w, newh, neww, self.interp)


class RandomFlip:
    def __init__(self, prob=0.5, *, horizontal=True, vertical=False):
        assert horizontal and not vertical
        self.prob = prob

    def get_transform(self, image):
        h, w = image.shape[:2]
        assert np.random.uniform() < self.prob          # (prob = 1.0 in the reference: always)
        return HFlipTransform(w)


class AugInput:
    def __init__(self, image, *, boxes=None, sem_seg=None):
        self.image = image

    def transform(self, tfm):
        self.image = tfm.apply_image(self.image)


class AugmentationList:
    def __init__(self, augs):
        self.augs = list(augs)

    def __call__(self, aug_input):
        tfms = []
        for a in self.augs:
            t = a.get_transform(aug_input.image)
            aug_input.transform(t)
            tfms.append(t)
        return TransformList(tfms)


def install_transforms():
    m = d2._mod("detectron2.data.transforms")
    m.ResizeShortestEdge, m.RandomFlip, m.AugmentationList, m.AugInput = ResizeShortestEdge, RandomFlip, AugmentationList, AugInput
    return m


# ================================================================================================ the cases
def run_case(out, name, seed=None):
    model_case = tta_ref.CASE_MODEL[name]
    min_sizes, max_size, flip = tta_ref.CASE_AUG[name]
    cfg, model, sup, weak, perms, masks = S.step_inputs(model_case)
    p = S.oracle_params(model)
    ocfg = S.oracle_cfg(cfg)
    roi_cls, pred_cls = cfg.MODEL.ROI_HEADS.NAME, cfg.MODEL.ROI_HEADS.FAST_RCNN.NAME
    mask_cls = cfg.MODEL.ROI_MASK_HEAD.NAME if cfg.MODEL.MASK_ON else None
    ref, _ = G.build_reference_model(p, ocfg, perms, roi_cls=roi_cls, pred_cls=pred_cls, mask_cls=mask_cls)
    ref.roi_heads.visual_threshold = ocfg["visual_threshold"]
    ref.roi_heads.box_predictor._freeze_layers(list(cfg.MODEL.FREEZE_LAYERS.FAST_RCNN))
    # what Detectron2 builds for PrecomputedProposals, and the TTA configuration
    ref.proposal_generator = None
    ref.test_augmentations = types.SimpleNamespace(ENABLED=True, MIN_SIZES=min_sizes, MAX_SIZE=max_size, FLIP=flip)
    ref.tta = ref._init_tta_fn(ref.test_augmentations)
    ref.eval()
    H, W = S.HW
    boxes = tta_ref.make_proposals(SEEDS[name] if seed is None else seed, H, W)
    image = sup[0]["image"]
    inp = {"file_name": "synthetic", "image_id": 0, "image": image, "height": 2 * H, "width": 2 * W,
           "proposals": d2.Instances((H, W), proposal_boxes=d2.Boxes(torch.from_numpy(boxes)), objectness_logits=torch.zeros(len(boxes)))}
    cap = {}
    bp = ref.roi_heads.box_predictor
    orig_predict_boxes = bp.predict_boxes

    def predict_boxes(predictions, proposals):
        cap["probs_sum"], cap["delta_mean"] = predictions[0][0].clone(), predictions[1].clone()
        return orig_predict_boxes(predictions, proposals)
    bp.predict_boxes = predict_boxes

    def fast_rcnn_inference(bxs, scores, image_shapes, score_thresh, nms_thresh, topk):
        cap["thresholds"] = (score_thresh, nms_thresh, topk)
        res, inds = [], []
        for b, s, shp in zip(bxs, scores, image_shapes):
            bb, ss, cc, rr = orc.fast_rcnn_inference_single(b, s, shp, score_thresh, nms_thresh, topk)
            res.append(d2.Instances(shp, pred_boxes=d2.Boxes(bb), scores=ss, pred_classes=cc))
            inds.append(rr)
        return res, inds
    G.REF["meta"].fast_rcnn_inference = fast_rcnn_inference
    with torch.no_grad():
        views = ref.tta(inp)
        if mask_cls is not None:
            # A FINDING, recorded instead of detections: the reference's TTA cannot run on its mask ROI heads. Under tta=True the predictor returns
            # [scores, deltas] (fast_rcnn.py:457-458), and WSROIHeadNoMetaWithMask._forward_box / WSROIHeadWithMaskFineTune._forward_box then stop at
            # `assert len(pred_instances) == 1` (roi_heads.py:770 / :882) because the similarity dictionary is never None in eval mode.
            import traceback
            try:
                ref.inference([inp])
                raised = None
            except AssertionError as e:
                raised = traceback.extract_tb(e.__traceback__)[-1]
            assert raised is not None and raised.filename.endswith("roi_heads/roi_heads.py") and "len(pred_instances) == 1" in raised.line, raised
            res = None
        else:
            res = ref.inference([inp])[0]["instances"]
    plan = tta_ref.view_plan(H, W, min_sizes, max_size, flip)
    assert len(views) == len(plan)
    u8 = image.permute(1, 2, 0).numpy().astype(np.uint8)
    for i, (v, (nh, nw, fl)) in enumerate(zip(views, plan)):
        assert tuple(v["image"].shape[1:]) == (nh, nw) and tuple(v["proposals"].image_size) == (nh, nw), (i, v["image"].shape, nh, nw)
        vb = v["proposals"].proposal_boxes.tensor.numpy()
        assert vb.dtype == np.float32
        assert np.array_equal(vb, tta_ref.view_boxes(boxes, H, W, nh, nw, fl)), (name, i)          # the stated rule IS what the transforms compute
        out[f"{name}/view_boxes{i}"] = vb
        if name == "tta" and not fl:
            vi = v["image"].permute(1, 2, 0).numpy()
            assert np.array_equal(vi, vi.astype(np.uint8).astype(vi.dtype))
            out[f"{name}/view_image{i}"] = vi.astype(np.uint8)
            if (nh, nw) == (H, W):
                assert np.array_equal(out[f"{name}/view_image{i}"], u8)          # no resampling pass when the size is unchanged
    out[f"{name}/views"] = np.array([[nh, nw, int(fl)] for nh, nw, fl in plan], np.int64)
    out[f"{name}/proposals"] = boxes
    if res is None:
        out[f"{name}/reference_raises_at"] = np.array(raised.lineno)
        print(name, "the reference raises at roi_heads.py:%d (%s)" % (raised.lineno, raised.line))
        return
    out[f"{name}/probs_sum"], out[f"{name}/delta_mean"] = G.npy(cap["probs_sum"]), G.npy(cap["delta_mean"])
    out[f"{name}/boxes"], out[f"{name}/scores"], out[f"{name}/classes"] = G.npy(res.pred_boxes.tensor), G.npy(res.scores), G.npy(res.pred_classes)
    out[f"{name}/has_masks"] = np.array(int(res.has("pred_masks")))
    out[f"{name}/thresholds"] = np.array(cap["thresholds"], np.float64)
    assert not res.has("pred_masks")
    thr, nms_thr, topk = cap["thresholds"]
    m = tta_ref.detection_margins(out[f"{name}/probs_sum"], out[f"{name}/delta_mean"], boxes, (H, W), bp.box2box_transform.weights, thr, nms_thr, int(topk))
    print(name, len(res), "detections; views", plan, "margins", m, "max score", float(res.scores.max()))
    assert m["score"] >= tta_ref.MARGIN and m["iou"] >= tta_ref.MARGIN and m["topk"] >= tta_ref.MARGIN, (name, m)
    assert len(res) > 3
    # postprocess drops nothing here or, if it does, the margin count is an upper bound; the recorded count is the reference's
    assert len(res) <= m["n"]


def main(path=OUT):
    install_transforms()
    G.load_meta_arch()
    out = {}
    for name in tta_ref.CASES:
        run_case(out, name)
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
