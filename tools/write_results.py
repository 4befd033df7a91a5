#!/usr/bin/env python
"""tools/write_results.py — tools/test_net.py, results only:

    python tools/write_results.py --config-file e2e_keypoint_rcnn_R_50_FPN_1x.yaml [--ckpt FILE] OUTPUT_DIR out [KEY VALUE ...]

Runs the detector over the test data and writes the detections as COCO result files (bbox.json, segm.json, keypoints.json,
as the config has the heads) to OUTPUT_DIR/inference/<dataset>/.  Nothing is evaluated: no evaluator is built and the
targets are not read, so this is the way to run the keypoint config (OKS is not built) and test sets whose json has no
annotations.  tools/test_net.py with OUTPUT_DIR set writes the same files next to its tables.

This is tools/test_net.py's own main() with its `inference` called with evaluate=False: every option, the config dump, the
checkpoint rules and the dataset loop are test_net.py's, whatever they become.  Not a reference tool."""
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_net  # noqa: E402


def main(argv=None):
    """-> per dataset {iou type: path of its file}"""
    run = test_net.inference
    test_net.inference = functools.partial(run, evaluate=False)
    try:
        return test_net.main(argv)
    except ValueError as e:
        if "output_folder" not in str(e):
            raise
        raise SystemExit("tools/write_results.py writes files only: set OUTPUT_DIR")
    finally:
        test_net.inference = run


if __name__ == "__main__":
    main()
