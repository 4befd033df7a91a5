#!/usr/bin/env python
"""tools/evaluate_keypoints.py — score a keypoint model, or a saved `keypoints.json`, under object keypoint similarity:

    python tools/evaluate_keypoints.py --config-file e2e_keypoint_rcnn_R_50_FPN_1x.yaml [--ckpt FILE] [KEY VALUE ...]
    python tools/evaluate_keypoints.py --config-file e2e_keypoint_rcnn_R_50_FPN_1x.yaml --results DIR [KEY VALUE ...]

Without --results it is tools/test_net.py's own main() (every option, the config dump, the checkpoint rules and the
dataset loop are test_net.py's) with its `inference` called with iou_types=("bbox",), keypoint_oks=True: the bbox and the
keypoints tables, and with OUTPUT_DIR set bbox.json and keypoints.json in OUTPUT_DIR/inference/<dataset>/.  With --results
the model is not run: DIR/keypoints.json (this project's or another tool's) is matched against DATASETS.TEST on
MODEL.DEVICE and the keypoints table is printed; with OUTPUT_DIR set, coco_results.pth / coco_results.txt go into DIR.

The rules (include/detops.h, "Keypoint evaluation (OKS)") are a restatement of pycocotools that nobody has checked against
it.  Not a reference tool: tools/test_net.py itself still refuses a keypoint config, the generic `keypoints` IoU type is
not routed to OKS yet."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_net  # noqa: E402

from evaluate_results import score_folder  # noqa: E402
from maskrcnn_benchmark.data.datasets.evaluation.keypoint_oks import evaluate_keypoint_file  # noqa: E402


def main(argv=None):
    """-> per dataset the COCOResults (rows bbox and keypoints; with --results the keypoints row alone)"""
    ap = argparse.ArgumentParser(description="Keypoint R-CNN evaluation under OKS")
    ap.add_argument("--config-file", default="e2e_keypoint_rcnn_R_50_FPN_1x.yaml", metavar="FILE")
    ap.add_argument("--local_rank", type=int, default=0)
    ap.add_argument("--ckpt", default=None, help="checkpoint to test (default: MODEL.WEIGHT, else the run's last checkpoint)")
    ap.add_argument("--images", type=int, default=16, help="synthetic test images")
    ap.add_argument("--results", default=None, metavar="DIR", help="score DIR/keypoints.json instead of running the model")
    ap.add_argument("opts", default=None, nargs=argparse.REMAINDER, help="KEY VALUE config overrides")
    args = ap.parse_args(argv)
    if args.results is None:
        forwarded = ["--config-file", args.config_file, "--local_rank", str(args.local_rank), "--images", str(args.images)]
        forwarded += ["--ckpt", args.ckpt] if args.ckpt is not None else []
        run = test_net.inference
        test_net.inference = lambda *a, **kw: run(*a, **dict(kw, iou_types=("bbox",), keypoint_oks=True))
        try:
            return test_net.main(forwarded + list(args.opts or []))
        finally:
            test_net.inference = run
    return score_folder("evaluate_keypoints.py", args, ("keypoints",),
                        lambda dataset, files, **kw: evaluate_keypoint_file(dataset, files["keypoints"], **kw))


if __name__ == "__main__":
    main()
