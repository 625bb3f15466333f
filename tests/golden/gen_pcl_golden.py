"""Generates tests/golden/pcl_golden.npz by RUNNING THE REFERENCE'S OWN weak detector with TYPE "PCL" (imported by file through d2_stubs,
as gen_unit_golden.py does): WeakDetectorOutputsBase(weak_detector_type="PCL").losses (weak_detector_fast_rcnn.py:189-238), whose
compute_pcl_loss_inputs (:488-519: get_graph_centers with sklearn's KMeans, the IoU graph and the greedy clustering, then
label_and_sample_proposals) is recorded per refinement iteration, and whose PCLFunction losses (pcl_loss.py:6-61) are differentiated back to
the refinement logits. Per case and iteration the file holds the logits, the reference's PCL decisions (labels, cls_weights,
gt_assignment, pc_labels, pc_count, img_cls_weights, pc_probs per image), loss_oicr_{k+1} and d(total loss)/d(logits).
Cases: VOC K=20 and COCO K=80 with two images, an image with fewer than 3 proposals, a single gt class, several classes, and an image
whose proposals repeat one box (two clusters on one box: a cluster with pc_count 0, a NaN loss, as the reference computes it).
Run here:  python tests/golden/gen_pcl_golden.py [out_dir]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import d2_stubs as d2  # noqa: E402

REF = d2.load_reference()
KEYS = ("labels", "cls_weights", "gt_assignment", "pc_labels", "pc_count", "img_cls_weights", "pc_probs")
CENTERS = torch.tensor([[100.0, 90.0, 120.0, 100.0], [280.0, 180.0, 150.0, 140.0], [200.0, 120.0, 60.0, 200.0]])


def npy(t):
    return t.detach().cpu().numpy()


def clustered_boxes(g, n, w=400.0, h=300.0):
    """proposals scattered around a few centres: every IoU band and many equal graph degrees occur"""
    c = CENTERS[torch.randint(0, len(CENTERS), (n,), generator=g)]
    jit = (torch.rand(n, 4, generator=g) - 0.5) * torch.tensor([30.0, 30.0, 60.0, 60.0])
    cx, cy = c[:, 0] + jit[:, 0], c[:, 1] + jit[:, 1]
    bw, bh = (c[:, 2] + jit[:, 2]).clamp(min=8), (c[:, 3] + jit[:, 3]).clamp(min=8)
    b = torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    b[:, 0::2] = b[:, 0::2].clamp(0, w)
    b[:, 1::2] = b[:, 1::2].clamp(0, h)
    return b


def case(out, tag, K, sizes, targets, seed, D=32, repeat_box=False):
    g = torch.Generator().manual_seed(seed)
    head = REF["weak"].WeakDetectorOutputsBase(
        d2.ShapeSpec(channels=D), box2box_transform=d2.Box2BoxTransform((10.0, 10.0, 5.0, 5.0)), num_classes=K, oicr_iter=3,
        fg_threshold=0.5, bg_threshold=0.1, weak_detector_type="PCL",
        proposal_matcher=REF["matcher"].Matcher([0.5], [0, 1], allow_low_quality_matches=False), test_score_thresh=0.05,
        base_classes=[c for c in range(K) if c % 4], novel_classes=[c for c in range(K) if c % 4 == 0])
    with torch.no_grad():
        for p_ in head.parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * (0.5 if p_.dim() > 1 else 0.1))
    head.train()
    boxes = [clustered_boxes(g, n) for n in sizes]
    if repeat_box:
        boxes[0][1::2] = boxes[0][0]
    props = [d2.Instances((300, 400), proposal_boxes=d2.Boxes(b), objectness_logits=torch.zeros(len(b))) for b in boxes]
    x = torch.randn(sum(sizes), D, generator=g)
    rec, orig = [], head.compute_pcl_loss_inputs

    def spy(*a, **k):
        r = orig(*a, **k)
        rec.append({key: [t.clone() for t in r[key]] for key in KEYS})
        return r
    head.compute_pcl_loss_inputs = spy
    preds, _ = head(x)
    for t in preds[2]:
        t.retain_grad()
    losses = head.losses(preds, props, [torch.tensor(t) for t in targets])
    sum(losses.values()).backward()
    out[f"{tag}/sizes"] = np.array(sizes)
    for i, b in enumerate(boxes):
        out[f"{tag}/boxes{i}"] = npy(b)
        out[f"{tag}/targets{i}"] = np.array(sorted(set(targets[i])))
    for k in range(3):
        out[f"{tag}/it{k}/logits"] = npy(preds[2][k])
        out[f"{tag}/it{k}/grad_logits"] = npy(preds[2][k].grad)
        out[f"{tag}/it{k}/loss"] = npy(losses[f"loss_oicr_{k + 1}"])
        for key in KEYS:
            for i, t in enumerate(rec[k][key]):
                out[f"{tag}/it{k}/{key}{i}"] = npy(t)
    print(tag, {k: round(float(v), 6) for k, v in losses.items()})


def main(out_dir=HERE):
    torch.set_num_threads(1)
    out = {}
    case(out, "P20", 20, [57, 33], [[3, 7, 12], [0]], 201)
    case(out, "P20n", 20, [2, 25], [[4], [1, 2, 2]], 202)
    case(out, "P80", 80, [64, 120], [[0, 17, 41, 79], [5, 6]], 203)
    case(out, "P20r", 20, [30, 20], [[3, 9, 14], [8]], 204, repeat_box=True)
    os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(out_dir, "pcl_golden.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
