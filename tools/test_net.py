#!/usr/bin/env python
"""tools/test_net.py — the reference's command line (tools/test_net.py:27-47):

    python tools/test_net.py --config-file e2e_mask_rcnn_R_50_FPN_1x.yaml [--ckpt FILE] [KEY VALUE ...]

Runs the detector over the test data and prints the COCO-style bbox (and segm) tables; with OUTPUT_DIR set they are
written to OUTPUT_DIR/inference/<dataset>/.  Data is the synthetic COCO-shaped generator (no network / datasets), `--images`
of it (not a reference option).  Single process only.  With random weights the AP is near 0: that is expected."""
import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "maskrcnn-benchmark_amd"))

import torch  # noqa: E402

from maskrcnn_benchmark.data import make_data_loader  # noqa: E402
from maskrcnn_benchmark.engine.bench_step import choose_layout, load_cfg  # noqa: E402
from maskrcnn_benchmark.engine.inference import inference  # noqa: E402
from maskrcnn_benchmark.modeling.detector import build_detection_model  # noqa: E402
from maskrcnn_benchmark.utils.checkpoint import DetectronCheckpointer  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description="MI355X-native Mask R-CNN inference and evaluation")
    ap.add_argument("--config-file", default="e2e_mask_rcnn_R_50_FPN_1x.yaml", metavar="FILE")
    ap.add_argument("--local_rank", type=int, default=0)
    ap.add_argument("--ckpt", default=None, help="checkpoint to test (default: MODEL.WEIGHT, else the run's last checkpoint)")
    ap.add_argument("--images", type=int, default=16, help="synthetic test images")
    ap.add_argument("opts", default=None, nargs=argparse.REMAINDER, help="KEY VALUE config overrides")
    args = ap.parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("tools/test_net.py is single-process only (WORLD_SIZE=%s): run it without a distributed launcher"
                         % os.environ["WORLD_SIZE"])
    cfg = load_cfg(args.config_file, args.opts or [])
    device = torch.device(cfg.MODEL.DEVICE)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s: %(message)s")
    logger = logging.getLogger("maskrcnn_benchmark")
    logger.info("Running with config:\n%s", cfg.dump())
    model = build_detection_model(cfg).to(device)
    layout = choose_layout(cfg, device)
    if layout != "nchw":
        model.set_channels_last(True, heads=layout == "all")
    out_dir = cfg.OUTPUT_DIR if cfg.OUTPUT_DIR != "." else ""
    checkpointer = DetectronCheckpointer(cfg, model, save_dir=out_dir)
    checkpointer.load((cfg.MODEL.WEIGHT if args.ckpt is None else args.ckpt) or None, use_latest=args.ckpt is None)
    iou_types = ("bbox",)
    if cfg.MODEL.MASK_ON:
        iou_types = iou_types + ("segm",)
    if cfg.MODEL.KEYPOINT_ON:
        iou_types = iou_types + ("keypoints",)
    dataset_names = cfg.DATASETS.TEST or ("synthetic_coco",)
    results = []
    for name in dataset_names:
        folder = os.path.join(out_dir, "inference", name) if out_dir else None
        loader = make_data_loader(cfg, is_train=False, length=args.images)
        res = inference(model, loader, dataset_name=name, iou_types=iou_types,
                        box_only=False if cfg.MODEL.RETINANET_ON else cfg.MODEL.RPN_ONLY, device=cfg.MODEL.DEVICE,
                        expected_results=cfg.TEST.EXPECTED_RESULTS, expected_results_sigma_tol=cfg.TEST.EXPECTED_RESULTS_SIGMA_TOL,
                        output_folder=folder)
        print(res)
        results.append(res)
    return results


if __name__ == "__main__":
    main()
