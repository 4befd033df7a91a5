#!/usr/bin/env python
"""tools/test_net.py seconds per image with and without the augmentation of
configs/test_time_aug/e2e_faster_rcnn_R_50_FPN_1x.yaml (profiles/bbox_aug_test_net.txt):

    python tools/bbox_aug_timing.py [--images 4] [--out FILE]

Writes a COCO-json set of `--images` generated 640 x 480 PNGs (80 categories) to a temporary directory, registers it and
calls tools/test_net.py's main() on it, Faster R-CNN R-50-FPN fp32 with random weights, two images per batch, no loader
workers.  Every configuration runs twice in this process: the first run pays MIOpen's kernel selection once per input
shape (18 passes = 18 shapes), the second is the figure.  The lines are the evaluation loop's own log."""
import argparse
import json
import logging
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "maskrcnn-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def write_set(root, count):
    from PIL import Image

    rng = np.random.RandomState(0)
    images, ann = [], []
    yy, xx = np.mgrid[0:480, 0:640]
    for i in range(1, count + 1):
        name = "img%d.png" % i
        a = np.clip(np.stack([xx * 0.4, yy * 0.5, 128 + 100 * np.sin(0.05 * xx + 0.03 * yy + i)], 2) + rng.normal(0, 20, (480, 640, 3)), 0, 255)
        Image.fromarray(a.astype(np.uint8), "RGB").save(os.path.join(root, name))
        images.append({"id": i, "file_name": name, "width": 640, "height": 480})
        ann.append({"id": i, "image_id": i, "category_id": 1, "bbox": [100.0, 80.0, 200.0, 150.0], "area": 30000.0, "iscrowd": 0,
                    "segmentation": [[100, 80, 300, 80, 300, 230, 100, 230]]})
    path = os.path.join(root, "instances.json")
    with open(path, "w") as f:
        json.dump({"images": images, "annotations": ann, "categories": [{"id": k, "name": "c%d" % k} for k in range(1, 81)]}, f)
    return path


class _Keep(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args(argv)
    import test_net
    from maskrcnn_benchmark.config.paths_catalog import DatasetCatalog

    root = tempfile.mkdtemp()
    DatasetCatalog.register("generated_coco", write_set(root, args.images), root)
    keep = _Keep()
    logging.getLogger("maskrcnn_benchmark.inference").addHandler(keep)
    opts = ["DATASETS.TEST", "('generated_coco',)", "TEST.IMS_PER_BATCH", "2", "DATALOADER.NUM_WORKERS", "0"]
    lines = []
    for label, yaml in (("plain", "e2e_faster_rcnn_R_50_FPN_1x.yaml"),
                        ("bbox_aug (18 passes)", "test_time_aug/e2e_faster_rcnn_R_50_FPN_1x.yaml")):
        for run in (1, 2):
            del keep.lines[:]
            t0 = time.time()
            test_net.main(["--config-file", yaml] + opts)
            took = time.time() - t0
            lines += ["%-22s run %d: %s" % (label, run, line) for line in keep.lines if "s / img" in line]
            lines.append("%-22s run %d: tools/test_net.py main() %.1f s in all (model build included)" % (label, run, took))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("python tools/bbox_aug_timing.py --images %d\n\n" % args.images + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
