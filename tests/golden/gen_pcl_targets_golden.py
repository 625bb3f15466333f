"""Generates tests/golden/pcl_targets_golden.npz by RUNNING THE REFERENCE'S OWN weak detector with TYPE "PCL" (gen_pcl_golden.py's set-up:
same head, same boxes, same seeds for the four shared cases) TWICE per case: as it is (`ref/...`) and with torch.Tensor.argsort replaced
by a stable sort (`stable/...`, the project's canonical rule; the reference's text is not touched). Recorded per case:
the head's parameters and input features, the classifier / detection logits, the boxes and targets, and per refinement iteration the two
probability matrices exactly as compute_pcl_loss_inputs receives them, its seven outputs per image, the loss and the logits gradient.

Space rules (the file stays under 1 MB; float32 throughout, the integer outputs as int32):
  * `it{k}/probs` is stored for k = 0 only (the MIL scores); for k >= 1 it IS `it{k-1}/probs_next` (the same softmax of the same tensor);
  * a `ref/...` array is stored only where it differs from `stable/...`: absent means equal. `it{k}/tie_free{i}` says whether all seven
    outputs of that (iteration, image) unit agree between the two runs;
  * the four shared cases (P20, P20n, P80, P20r) do not repeat pcl_golden.npz: their refinement logits, losses and gradients are asserted
    equal to that file here and read from it by the tests;
  * the large cases (`sparse` = 1) hold no logits and no gradients, and their probability matrices only at the columns the targets read
    (the image's classes, `it{k}/cols{i}`): every other column never enters compute_pcl_loss_inputs.

The generator asserts, and fails otherwise: every k-means fit at the reference's call site equals pcl_kmeans.top_ranking; every unit keeps
its integer decisions under six relative 2^-21 perturbations of both probability inputs (stable run); at least 36 units are tie-free,
among them every unit of the six small cases (C1).
Run here:  python tests/golden/gen_pcl_targets_golden.py [out_dir]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_pcl_golden as gp  # noqa: E402
import pcl_kmeans as pk  # noqa: E402

d2, REF, KEYS, npy = gp.d2, gp.REF, gp.KEYS, gp.npy
INT_KEYS = ("labels", "gt_assignment", "pc_labels", "pc_count")
SHARED = ("P20", "P20n", "P80", "P20r")
_ARGSORT = torch.Tensor.argsort


def _stable_argsort(self, dim=-1, descending=False, stable=True):
    return torch.sort(self, dim=dim, descending=descending, stable=True)[1]


def build(K, sizes, seed, scale, D=32, repeat_box=False):
    g = torch.Generator().manual_seed(seed)
    head = REF["weak"].WeakDetectorOutputsBase(
        d2.ShapeSpec(channels=D), box2box_transform=d2.Box2BoxTransform((10.0, 10.0, 5.0, 5.0)), num_classes=K, oicr_iter=3,
        fg_threshold=0.5, bg_threshold=0.1, weak_detector_type="PCL",
        proposal_matcher=REF["matcher"].Matcher([0.5], [0, 1], allow_low_quality_matches=False), test_score_thresh=0.05,
        base_classes=[c for c in range(K) if c % 4], novel_classes=[c for c in range(K) if c % 4 == 0])
    with torch.no_grad():
        for p_ in head.parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * ((0.5 if p_.dim() > 1 else 0.1) * scale / 0.5))
    head.train()
    boxes = [gp.clustered_boxes(g, n) for n in sizes]
    if repeat_box:
        boxes[0][1::2] = boxes[0][0]
    props = [d2.Instances((300, 400), proposal_boxes=d2.Boxes(b), objectness_logits=torch.zeros(len(b))) for b in boxes]
    x = torch.randn(sum(sizes), D, generator=g)
    return head, boxes, props, x


def run(K, sizes, targets, seed, scale, repeat_box, stable, stats):
    head, boxes, props, x = build(K, sizes, seed, scale, repeat_box=repeat_box)
    rec, calls, orig, orig_top = [], [], head.compute_pcl_loss_inputs, head.get_top_ranking_proposals
    checking = [True]

    def top(probs, *a, **k):
        r = orig_top(probs, *a, **k)
        if checking[0]:
            mine = pk.top_ranking(probs.detach().numpy().reshape(-1))
            got = np.atleast_1d(npy(r)).reshape(-1)
            stats["fits"] += 1
            stats["fits_over_16"] += len(got) > 16
            stats["max_top"] = max(stats["max_top"], len(got))
            assert np.array_equal(np.sort(got), mine), f"k-means restatement differs from scikit-learn at N = {probs.shape[0]}"
        return r

    def spy(*a, **k):
        r = orig(*a, **k)
        rec.append({key: [t.clone() for t in r[key]] for key in KEYS})
        calls.append([a[0], a[1].clone(), a[2], a[3].clone(), a[4]])
        return r
    head.get_top_ranking_proposals = top
    head.compute_pcl_loss_inputs = spy
    torch.Tensor.argsort = _stable_argsort if stable else _ARGSORT
    try:
        preds, _ = head(x)
        for t in preds[2]:
            t.retain_grad()
        losses = head.losses(preds, props, [torch.tensor(t) for t in targets])
        sum(losses.values()).backward()
        if stable:                      # decisions keep their margin: six relative 2^-21 perturbations of both inputs
            g = torch.Generator().manual_seed(seed + 1000)
            checking[0] = False
            for k, (pr, p0, gc, p1, ind) in enumerate(calls):
                for _ in range(6):
                    e0 = 1 + (torch.rand(p0.shape, generator=g) * 2 - 1) * 2.0 ** -21
                    e1 = 1 + (torch.rand(p1.shape, generator=g) * 2 - 1) * 2.0 ** -21
                    with torch.no_grad():
                        r = orig(pr, p0 * e0, gc, p1 * e1, ind)
                    stats["perturbed"] += len(sizes)
                    for key in INT_KEYS:
                        for i in range(len(sizes)):
                            assert torch.equal(r[key][i], rec[k][key][i]), f"iteration {k} image {i}: {key} moves under a 2^-21 perturbation"
    finally:
        torch.Tensor.argsort = _ARGSORT
    return dict(head=head, boxes=boxes, x=x, preds=preds, losses=losses, rec=rec, calls=calls)


def same(a, b):
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def case(out, tag, K, sizes, targets, seed, scale=0.5, repeat_box=False, sparse=False, stats=None, old=None):
    r = {False: run(K, sizes, targets, seed, scale, repeat_box, False, stats), True: run(K, sizes, targets, seed, scale, repeat_box, True, stats)}
    st = r[True]
    out[f"{tag}/sizes"] = np.array(sizes)
    out[f"{tag}/K"] = np.array(K)
    out[f"{tag}/sparse"] = np.array(int(sparse))
    for i, b in enumerate(st["boxes"]):
        out[f"{tag}/boxes{i}"] = npy(b)
        out[f"{tag}/targets{i}"] = np.array(sorted(set(targets[i])))
    if not sparse:
        out[f"{tag}/x"] = npy(st["x"])
        for name, p_ in st["head"].state_dict().items():
            out[f"{tag}/param/{name}"] = npy(p_)
        out[f"{tag}/classifier_logits"] = npy(st["preds"][0])
        out[f"{tag}/detection_logits"] = npy(st["preds"][1])
        out[f"{tag}/stable/loss_im_cls"] = npy(st["losses"]["loss_im_cls"])
    tie_free = []
    idx = np.insert(np.cumsum(sizes), 0, 0)
    for k in range(3):
        p0, p1 = npy(st["calls"][k][1]), npy(st["calls"][k][3])
        assert same(p0, npy(r[False]["calls"][k][1])) and same(p1, npy(r[False]["calls"][k][3]))
        if k > 0:
            assert same(p0, npy(st["calls"][k - 1][3]))
        if sparse:
            for i in range(len(sizes)):
                cols = out[f"{tag}/targets{i}"]
                out[f"{tag}/it{k}/cols{i}"] = cols
                if k == 0:
                    out[f"{tag}/it{k}/probs{i}"] = p0[idx[i]:idx[i + 1]][:, cols]
                out[f"{tag}/it{k}/probs_next{i}"] = p1[idx[i]:idx[i + 1]][:, cols]
        else:
            if k == 0:
                out[f"{tag}/it{k}/probs"] = p0
            out[f"{tag}/it{k}/probs_next"] = p1
        for run_, name in ((True, "stable"), (False, "ref")):
            q = r[run_]
            for key in KEYS:
                for i, t in enumerate(q["rec"][k][key]):
                    a = npy(t)
                    a = a.astype(np.int32) if key in INT_KEYS else a
                    if run_ or not same(a, out[f"{tag}/it{k}/stable/{key}{i}"]):
                        out[f"{tag}/it{k}/{name}/{key}{i}"] = a
            loss, grad, lg = npy(q["losses"][f"loss_oicr_{k + 1}"]), npy(q["preds"][2][k].grad), npy(q["preds"][2][k])
            if old is not None and tag in SHARED:
                if not run_:
                    assert same(lg, old[f"{tag}/it{k}/logits"]) and same(grad, old[f"{tag}/it{k}/grad_logits"]), tag
                    assert same(loss, old[f"{tag}/it{k}/loss"]), tag
                elif not sparse:
                    assert same(grad, npy(r[False]["preds"][2][k].grad)), tag
            elif not sparse:
                if run_:
                    out[f"{tag}/it{k}/logits"] = lg
                if run_ or not same(grad, out[f"{tag}/it{k}/stable/grad_logits"]):
                    out[f"{tag}/it{k}/{name}/grad_logits"] = grad
            if run_ or not same(loss, out[f"{tag}/it{k}/stable/loss"]):
                out[f"{tag}/it{k}/{name}/loss"] = loss
        for i in range(len(sizes)):
            free = all(same(npy(r[True]["rec"][k][key][i]), npy(r[False]["rec"][k][key][i])) for key in KEYS)
            out[f"{tag}/it{k}/tie_free{i}"] = np.array(int(free))
            tie_free.append(free)
    print(tag, {k: round(float(v), 6) for k, v in st["losses"].items()}, "tie-free units", sum(tie_free), "of", len(tie_free), flush=True)
    return tie_free


CASES = [
    ("P20", 20, [57, 33], [[3, 7, 12], [0]], 201, {}),
    ("P20n", 20, [2, 25], [[4], [1, 2, 2]], 202, {}),
    ("P80", 80, [64, 120], [[0, 17, 41, 79], [5, 6]], 203, {}),
    ("P20r", 20, [30, 20], [[3, 9, 14], [8]], 204, dict(repeat_box=True)),
    ("S16", 20, [16, 12], [[2, 11], [5]], 207, {}),
    ("S40", 20, [40, 24], [[1, 6, 19], [6, 13]], 208, {}),
    ("L20", 20, [300, 512], [[3, 7, 12], [0, 15]], 209, dict(sparse=True)),
    ("L20u", 20, [300, 512], [[3, 7, 12], [0, 15]], 210, dict(sparse=True, scale=0.05)),
    ("L80", 80, [400, 600], [[0, 17, 41, 79], [5, 6, 30]], 211, dict(sparse=True)),
]
SMALL = ("P20", "P20n", "P80", "P20r", "S16", "S40")


def main(out_dir=HERE):
    torch.set_num_threads(1)
    old = np.load(os.path.join(HERE, "pcl_golden.npz"))
    out, stats, free = {}, dict(fits=0, fits_over_16=0, max_top=0, perturbed=0), {}
    for tag, K, sizes, targets, seed, kw in CASES:
        free[tag] = case(out, tag, K, sizes, targets, seed, stats=stats, old=old, **kw)
    n_free = sum(sum(v) for v in free.values())
    print("fits checked against pcl_kmeans.top_ranking:", stats["fits"], "with more than 16 top-ranking rows:", stats["fits_over_16"],
          "largest top-ranking set:", stats["max_top"], "| perturbed unit-draws without a moved decision:", stats["perturbed"],
          "| tie-free units:", n_free, {k: f"{sum(v)}/{len(v)}" for k, v in free.items()})
    assert n_free >= 36 and all(all(free[t]) for t in SMALL), "C1: at least 36 tie-free units, among them every unit of the six small cases"
    out["tags"] = np.array([c[0] for c in CASES])
    os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(out_dir, "pcl_targets_golden.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
