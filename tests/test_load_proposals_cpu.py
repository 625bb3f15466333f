"""MODEL.LOAD_PROPOSALS without a GPU: the default, the ROI heads' row count with the switch off and on, the refusals (naming key and limit,
at construction for an RPN model and at the call for proposals handed in), and the recorded reference run
(tests/golden/load_proposals_golden.npz, gen_load_proposals_golden.py) against the oracle's parts composed on ALL rows of the weak images:
roi_align, res5_head, weak_head_forward_train, weak_losses -- what the GPU test then holds the kernels to."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import unit_oracle as orc
from unit_amd import config
from unit_amd.modeling import build_model
from unit_amd.modeling.inference import UnsupportedConfig

HERE = os.path.dirname(__file__)
FX = np.load(os.path.join(HERE, "golden", "load_proposals_golden.npz"))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_load_proposals_golden", os.path.join(HERE, "golden", "gen_load_proposals_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _cfg(load, post=50, typ="OICR"):
    c = config.voc_rcnn_c4_split1(50)
    c.MODEL.DEVICE = "cpu"
    c.MODEL.LOAD_PROPOSALS = load
    c.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 16
    c.MODEL.RPN.PRE_NMS_TOPK_TRAIN, c.MODEL.RPN.POST_NMS_TOPK_TRAIN = 300, post
    c.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.TYPE = typ
    return c


def test_config_default_is_off():
    for c in (config.voc_rcnn_c4_split1(50), config.voc_rcnn_c4_split1(101), config.voc_rcnn_c4_split1_ft(50)):
        assert c.MODEL.LOAD_PROPOSALS is False
    assert build_model(_cfg(False)).roi_heads.load_proposals is False


def test_weak_rows_per_image_off_and_on():
    props = torch.zeros(2, 1500, 4)
    off = build_model(_cfg(False)).roi_heads
    assert off.weak_rows_per_image(props) == off.batch_size_per_image // off.weak_divisor == 16 // off.weak_divisor
    off.batch_size_per_image, off.weak_divisor = 512, 4
    assert off.weak_rows_per_image(props) == 128 and off.weak_rows_per_image(torch.zeros(2, 7, 4)) == 128
    on = build_model(_cfg(True)).roi_heads
    assert on.load_proposals is True
    assert on.weak_rows_per_image(props) == 1500 and on.weak_rows_per_image(torch.zeros(3, 50, 4)) == 50
    assert on.weak_rows_per_image(torch.zeros(1, 8192, 4)) == 8192


def test_refusals_name_the_key_and_the_limit():
    # at construction: an RPN model's weak images get POST_NMS_TOPK_TRAIN slots
    with pytest.raises(UnsupportedConfig) as e:
        build_model(_cfg(True, post=8193))
    assert "MODEL.LOAD_PROPOSALS" in str(e.value) and "8192" in str(e.value) and "POST_NMS_TOPK_TRAIN" in str(e.value) and "OICR" in str(e.value)
    with pytest.raises(UnsupportedConfig) as e:
        build_model(_cfg(True, post=2049, typ="PCL"))
    assert "MODEL.LOAD_PROPOSALS" in str(e.value) and "2048" in str(e.value) and "PCL" in str(e.value)
    assert build_model(_cfg(True, post=2048, typ="PCL")).roi_heads.load_proposals
    assert build_model(_cfg(True, post=8192)).roi_heads.load_proposals
    build_model(_cfg(False, post=9000))          # the switch off: no limit, the weak rows are the first S // divisor
    # at the call: the count arrives with the proposals
    oicr, pcl = build_model(_cfg(True)).roi_heads, build_model(_cfg(True, typ="PCL")).roi_heads
    with pytest.raises(UnsupportedConfig) as e:
        oicr.weak_rows_per_image(torch.zeros(2, 8193, 4))
    assert "MODEL.LOAD_PROPOSALS" in str(e.value) and "8192" in str(e.value) and "8193" in str(e.value)
    with pytest.raises(UnsupportedConfig) as e:
        pcl.weak_rows_per_image(torch.zeros(2, 2049, 4))
    assert "2048" in str(e.value) and "2049" in str(e.value)
    assert pcl.weak_rows_per_image(torch.zeros(2, 2048, 4)) == 2048 and oicr.weak_rows_per_image(torch.zeros(2, 2049, 4)) == 2049


def test_fixture_holds_what_it_says():
    assert [str(c) for c in FX["cases"]] == ["lp_oicr", "lp_reg", "lp_pcl"] and FX["weak_sizes"].tolist() == [1100, 1500]
    gen = _gen()
    for i, b in enumerate(gen.weak_boxes()):          # the stored proposals are the seeded ones; inside the image, not degenerate
        assert np.array_equal(FX[f"weak_boxes{i}"], b.numpy()) and len(b) == gen.WEAK_SIZES[i] > 1024
        assert float(b.min()) >= 0 and float(b[:, 2].max()) <= 128 and float(b[:, 3].max()) <= 96
        assert float((b[:, 2] - b[:, 0]).min()) >= 6 and float((b[:, 3] - b[:, 1]).min()) >= 6
    base = ["loss_box_reg", "loss_cls", "loss_im_cls", "loss_oicr_1", "loss_oicr_2", "loss_oicr_3"]
    for case, extra, calls in (("lp_oicr", [], 3), ("lp_reg", ["loss_regression_bbox", "loss_regression_cls"], 4), ("lp_pcl", [], 0)):
        assert [str(n) for n in FX[f"{case}/loss_names"]] == sorted(base + extra + ["loss_rpn_cls", "loss_rpn_loc"])
        assert np.isfinite(FX[f"{case}/losses"]).all() and (FX[f"{case}/losses"] > 0).all()
        assert sum(f"{case}/oicr_labels{k}" in FX.files for k in range(5)) == calls
        for k in range(calls):
            lab, w = FX[f"{case}/oicr_labels{k}"], FX[f"{case}/oicr_weights{k}"]
            assert lab.shape == w.shape == (2600,) and lab.min() >= 0 and lab.max() == 20 and (w >= 0).all()
            for sl in (slice(0, 1100), slice(1100, 2600)):          # foreground, weighted background and ignored rows in both images
                assert (lab[sl] < 20).any() and ((lab[sl] == 20) & (w[sl] > 0)).any() and (w[sl] == 0).any()
            assert (lab[128:1100] < 20).any() and (w[1100 + 1024:] > 0).any()          # past the rows the switch-off cut keeps, past 1024
        assert calls == 0 or any((FX[f"{case}/oicr_labels{k}"][1100 + 1024:] < 20).any() for k in range(calls))
    # the three cases share weights and data: what does not depend on the weak detector's type is the same number
    i = lambda case, n: FX[f"{case}/losses"][[str(x) for x in FX[f"{case}/loss_names"]].index(n)]
    assert i("lp_oicr", "loss_im_cls") == i("lp_pcl", "loss_im_cls") and i("lp_oicr", "loss_oicr_1") != i("lp_pcl", "loss_oicr_1")


def test_fixture_against_the_oracles_parts_on_all_rows():
    """roi_align -> res5_head -> weak_head_forward_train -> weak_losses on every given proposal reproduces the recorded weak losses; the
    oracle's per-iteration targets are the recorded labels (exactly) and weights. The same composition on the first 16 // divisor rows --
    what the code did before it honoured the switch -- does not."""
    gen = _gen()
    cfg, model, sup, weak, perms = gen.lp_inputs("lp_oicr")
    p = {k: v.detach().clone() for k, v in model.state_dict().items()}
    boxes = [torch.from_numpy(FX[f"weak_boxes{i}"]) for i in range(2)]
    targets = [x["instances"].gt_classes for x in weak]
    with torch.no_grad():
        wx, _ = orc.preprocess_image([x["image"] for x in weak], cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD)
        wfeat = orc.resnet_c4(wx, p, 50, "backbone.")

        def weak_half(bx):
            wbf = orc.res5_head(orc.roi_align(wfeat, orc.boxes_to_rois(bx)), p, "roi_heads.weak_box_head")
            cs, ds, oicr = orc.weak_head_forward_train(wbf, p, "roi_heads.box_predictor.weak_detector_head")
            return cs, ds, oicr, orc.weak_losses(cs, ds, oicr, bx, targets, num_classes=20)
        cs, ds, oicr, got = weak_half(boxes)
        names = [str(n) for n in FX["lp_oicr/loss_names"]]
        want = {n: float(FX["lp_oicr/losses"][names.index(n)]) for n in got}
        print({k: (float(v), want[k]) for k, v in got.items()})
        for k, v in got.items():
            assert abs(float(v) - want[k]) <= 1e-5 * max(1.0, abs(want[k])), (k, float(v), want[k])
        idx = [0, 1100, 2600]
        gtc = [torch.unique(t) for t in targets]
        xr = torch.cat([torch.softmax(cs[a:b], -1) * torch.softmax(ds[a:b], 0) for a, b in zip(idx, idx[1:])])
        for k in range(3):
            probs = xr if k == 0 else torch.softmax(oicr[k - 1], -1)
            lab, w = orc.oicr_targets(boxes, probs, gtc, idx, 0.5, 0.1, num_classes=20)
            assert np.array_equal(lab.numpy(), FX[f"lp_oicr/oicr_labels{k}"]), k
            assert np.allclose(w.numpy(), FX[f"lp_oicr/oicr_weights{k}"], rtol=1e-5, atol=1e-8), k
        sw = 16 // cfg.MODEL.ROI_HEADS.WEAK_CLASSIFIER_PROPOSAL_DIVISOR
        *_, cut = weak_half([b[:sw] for b in boxes])
        assert any(abs(float(cut[k]) - want[k]) > 1e-3 * max(1.0, abs(want[k])) for k in cut)
