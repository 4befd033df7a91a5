#!/usr/bin/env python
"""tools/evaluate_results.py — score saved COCO result files without running the model:

    python tools/evaluate_results.py --config-file e2e_mask_rcnn_R_50_FPN_1x.yaml --results DIR [KEY VALUE ...]

DIR holds `bbox.json` and / or `segm.json`, as tools/test_net.py (OUTPUT_DIR/inference/<dataset>/), tools/write_results.py
or any other tool writes them.  The dataset is the one of DATASETS.TEST, built as tools/test_net.py builds it; the
detections are matched on MODEL.DEVICE.  Prints the same tables as tools/test_net.py and, with OUTPUT_DIR set, writes
coco_results.pth / coco_results.txt into DIR.  `keypoints.json` is not scored here: tools/evaluate_keypoints.py --results
scores it under OKS."""
import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "maskrcnn-benchmark_amd"))

from maskrcnn_benchmark.data import make_data_loader  # noqa: E402
from maskrcnn_benchmark.data.datasets.evaluation.coco_results import evaluate_result_files  # noqa: E402
from maskrcnn_benchmark.engine.bench_step import load_cfg  # noqa: E402


def score_folder(tool, args, iou_types, score):
    """The `--results` path of this tool and of tools/evaluate_keypoints.py: the config of args.config_file and args.opts,
    one dataset of DATASETS.TEST with args.images synthetic images, the <iou type>.json of `iou_types` that args.results
    holds -> [score(dataset, {iou type: path}, output_folder=, batch=, device=, expected_results=, ...)], printed."""
    cfg = load_cfg(args.config_file, args.opts or [])
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s: %(message)s")
    names = cfg.DATASETS.TEST or ("synthetic_coco",)
    if len(names) != 1:
        raise SystemExit("tools/%s scores one folder against one dataset: DATASETS.TEST names %d" % (tool, len(names)))
    files = {t: os.path.join(args.results, t + ".json") for t in iou_types}
    files = {t: p for t, p in files.items() if os.path.exists(p)}
    if not files:
        raise SystemExit("no %s in %s" % (" or ".join(t + ".json" for t in iou_types), args.results))
    dataset = make_data_loader(cfg, is_train=False, length=args.images).dataset
    out_dir = cfg.OUTPUT_DIR if cfg.OUTPUT_DIR != "." else ""
    res = score(dataset, files, output_folder=args.results if out_dir else None, batch=cfg.TEST.IMS_PER_BATCH,
                device=cfg.MODEL.DEVICE, expected_results=cfg.TEST.EXPECTED_RESULTS,
                expected_results_sigma_tol=cfg.TEST.EXPECTED_RESULTS_SIGMA_TOL)
    print(res)
    return [res]


def main(argv=None):
    ap = argparse.ArgumentParser(description="Score bbox.json / segm.json result files against DATASETS.TEST")
    ap.add_argument("--config-file", default="e2e_mask_rcnn_R_50_FPN_1x.yaml", metavar="FILE")
    ap.add_argument("--results", required=True, metavar="DIR", help="folder that holds bbox.json and / or segm.json")
    ap.add_argument("--images", type=int, default=16, help="synthetic test images (as tools/test_net.py)")
    ap.add_argument("opts", default=None, nargs=argparse.REMAINDER, help="KEY VALUE config overrides")
    return score_folder("evaluate_results.py", ap.parse_args(argv), ("bbox", "segm"), evaluate_result_files)


if __name__ == "__main__":
    main()
