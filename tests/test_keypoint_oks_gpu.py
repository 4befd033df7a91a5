"""csrc/eval_oks.hip on the device against the numpy path (_eval_cpu.eval_oks, pinned to the literal loops by
tests/test_keypoint_oks_cpu.py), at the smallest shapes at which the kernel can go wrong; and the evaluator on the device
against the CPU path.

Tolerance for OKS values: the derivation of tests/test_keypoint_oks_cpu.py, |a - b| <= 2 (K + 1) 2^-52, which takes each exp
within 1 ulp.  For the device's fp64 exp that figure is the one of ROCm's device-library (OCML) accuracy table as recalled:
the table is not installed with the ROCm tree this was written on, so it could not be read there; it is not looser than
the host's, and the bound is not widened.  Largest difference observed on an MI355X: profiles/keypoint_oks_tests.txt.
"""
import numpy as np
import pytest
import torch

import oks_refs as R
from maskrcnn_benchmark import _C
from maskrcnn_benchmark.data.datasets.evaluation import keypoint_oks as KO
from oks_refs import EMPTY, SEED, SHAPES, assert_clear_of_the_thresholds, oks_tolerance, run_op
from oks_refs import evaluate_boxlists as _evaluate

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = _C.EVAL_OKS_MAX_K


def _both(pb):
    """-> (device oks, device dt_area, numpy oks, numpy dt_area), the device's twice with equal bits"""
    oks, area = run_op(pb, DEV)
    oks2, area2 = run_op(pb, DEV)
    assert oks.tobytes() == oks2.tobytes() and area.tobytes() == area2.tobytes()
    return (oks, area) + run_op(pb)


@pytest.mark.parametrize("K", [1, 17, CAP, CAP + 1])
def test_device_against_numpy(K):
    pb = R.random_problems(200 + K, SHAPES, K, unlabelled=(1, 6))          # D = 0 and G = 0 between full problems; k1 == 0
    oks, area, ref, ref_area = _both(pb)
    diff = float(np.abs(oks - ref).max())
    print("K = %d: largest |device - numpy| = %.3g (bound %.3g), %d of %d differ" % (K, diff, oks_tolerance(K),
                                                                                    int((oks != ref).sum()), oks.size))
    assert oks.shape == ref.shape and diff <= oks_tolerance(K)
    np.testing.assert_array_equal(area, ref_area)
    if K > CAP:                                                            # the host path: the same numpy function
        assert diff == 0.0


@pytest.mark.parametrize("shapes", [[(1, 1)], [(9, 7)], [(5, 13)], [(1, 257)], [(257, 1)], [(3, 0), (21, 3), (0, 2), (1, 2)]],
                         ids=["1", "63", "65", "1x257", "257x1", "mixed"])
def test_pair_counts_across_wave_and_workgroup_edges(shapes):
    pb = R.random_problems(300 + len(shapes) + shapes[0][0], shapes, 17, unlabelled=(0,))
    oks, area, ref, ref_area = _both(pb)
    assert oks.size == sum(d * g for d, g in shapes)
    assert float(np.abs(oks - ref).max()) <= oks_tolerance(17)
    np.testing.assert_array_equal(area, ref_area)
    pb2 = dict(pb, dt_kpts=pb["dt_kpts"].copy())
    pb2["dt_kpts"][:, :, 2] = np.nan                                       # the detections' third column changes nothing
    oks2, area2 = run_op(pb2, DEV)
    assert oks2.tobytes() == oks.tobytes() and area2.tobytes() == area.tobytes()


def test_no_problem_and_exact_ones():
    empty = {"dt_kpts": np.zeros((0, 17, 3), np.float32), "gt_kpts": np.zeros((0, 17, 3), np.float32),
             "gt_boxes": np.zeros((0, 4), np.float32), "gt_area": np.zeros((0,)), "sigmas": np.array(R.SIGMAS),
             "dt_offset": np.zeros((1,), np.int32), "gt_offset": np.zeros((1,), np.int32), "iou_offset": np.zeros((1,), np.int64)}
    oks, area = run_op(empty, DEV)                                         # P = 0
    assert oks.shape == (0,) and area.shape == (0,)
    pb = R.random_problems(7, [(4, 0), (3, 0)], 17)                        # detections, no pair: the areas alone
    oks, area, _, ref_area = _both(pb)
    assert oks.shape == (0,) and area.shape == (7,)
    np.testing.assert_array_equal(area, ref_area)
    # every e is 0: exactly 1.0 on both sides (visible keypoints on the spot; no visible keypoint, inside the doubled box)
    pb = R.random_problems(8, [(2, 2)], 17, unlabelled=(1,))
    pb["dt_kpts"][0, :, :2] = pb["gt_kpts"][0, :, :2]
    pb["dt_kpts"][1, :, :2] = pb["gt_boxes"][1, None, :2]
    oks, _, ref, _ = _both(pb)
    assert oks[0] == 1.0 == ref[0] and oks[3] == 1.0 == ref[3] and oks[2] < 1.0


def _raw_call(pb, K, oks, area, guard):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    args = [t(pb[k]) for k in ("dt_kpts", "gt_kpts", "gt_boxes", "gt_area", "sigmas", "dt_offset", "gt_offset", "iou_offset")]
    P, D_total, total = len(pb["dt_offset"]) - 1, pb["dt_kpts"].shape[0], int(pb["iou_offset"][-1])
    rc = _C.lib.detops_eval_oks(*(a.data_ptr() for a in args[:5]), K, *(a.data_ptr() for a in args[5:]), P, D_total, total,
                                oks.data_ptr() + 8 * guard, area.data_ptr() + 8 * guard, _C.stream_of(oks))
    torch.cuda.synchronize()
    return rc


def test_guards_stay_untouched_and_the_entry_point_refuses_without_launching():
    guard = 8
    pb = R.random_problems(9, [(5, 13), (2, 0), (3, 3)], 17)
    total, D_total = int(pb["iou_offset"][-1]), pb["dt_kpts"].shape[0]
    oks = torch.full((total + 2 * guard,), -7.0, dtype=torch.float64, device=DEV)
    area = torch.full((D_total + 2 * guard,), -7.0, dtype=torch.float64, device=DEV)
    assert _raw_call(pb, 17, oks, area, guard) == 0
    ref, ref_area = run_op(pb)
    for buf, want in ((oks, ref), (area, ref_area)):
        got = buf.cpu().numpy()
        assert (got[:guard] == -7.0).all() and (got[-guard:] == -7.0).all()
        assert np.abs(got[guard:-guard] - want).max() <= oks_tolerance(17)
    # beyond the cap, and K < 1: a code, nothing written
    big = R.random_problems(9, [(2, 2)], CAP + 1)
    for problem, K, code in ((big, CAP + 1, -3), (pb, 0, -1)):
        oks.fill_(-7.0)
        area.fill_(-7.0)
        assert _raw_call(problem, K, oks, area, guard) == code
        assert bool((oks == -7.0).all()) and bool((area == -7.0).all())


def test_evaluator_on_the_device_against_the_cpu_path():
    images = R.random_images(SEED, n_images=8, empty=EMPTY)
    assert_clear_of_the_thresholds(images)                                 # on the numpy values: matches compare exactly
    cpu, dev = _evaluate(images), _evaluate(images, device=DEV)
    assert len(cpu.records["keypoints"]) == len(dev.records["keypoints"]) > 0
    for a, b in zip(dev.records["keypoints"], cpu.records["keypoints"]):
        assert (a["image"], a["category"]) == (b["image"], b["category"])
        for key in ("scores", "dt_match", "dt_ignore", "gt_ignore"):
            assert np.array_equal(a[key], b[key]), key
    stats = dev.summarize()["keypoints"]
    np.testing.assert_array_equal(stats, cpu.summarize()["keypoints"])
    np.testing.assert_allclose(stats, R.coco_stats(images, 3)[1], rtol=0, atol=1e-12)
    assert (dev.num_images, dev.num_detections, dev.num_groundtruths) == (cpu.num_images, cpu.num_detections, cpu.num_groundtruths)
    assert isinstance(dev, KO.KeypointOKSEvaluator) and 0.05 < stats[0] < 0.95
