"""Proposal recall (`box_only`) without a GPU: the numpy path and the kernel of csrc/eval_proposals.hip under the host emulation
against what the REFERENCE's evaluate_box_proposals returned (tests/golden/box_proposals_reference.npz), the streaming
evaluator, `inference(box_only=True)`, tools/test_net.py on the RPN-only config, and the entry point's argument checks.

Bounds.  The matched overlaps are fp32 values made by the same IEEE operations in the same order on every path, and the
matching compares them exactly: `gt_overlaps` is compared bit for bit, `num_pos` and `recalls` (a count divided by a count,
one fp32 division) exactly.  `ar` is the mean of the ten fp32 recalls: the same ten numbers added in another order differ by at
most nine roundings of partial sums below 10, divided by 10, plus the division's own rounding: |ar - reference| <= 10 * 2^-24.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import box_proposal_cases as C
import cpu_shim
from maskrcnn_benchmark import _C, _abi
from maskrcnn_benchmark.data.datasets import evaluation as E
from maskrcnn_benchmark.data.datasets.evaluation import box_proposals as BP
from maskrcnn_benchmark.structures.bounding_box import BoxList

AR_TOL = 10 * 2.0 ** -24


@pytest.fixture(scope="module")
def fx():
    return C.load_fixture()


def _evaluate(fx, batch, limits=C.LIMITS, areas=C.AREAS, device="cpu"):
    ev = BP.BoxProposalEvaluator(limits, areas)
    return E._feed(ev, C.fixture_predictions(fx, device), C.FixtureDataset(fx), batch, device)


def _assert_reference(fx, results):
    assert list(results) == [(limit, area) for limit in C.LIMITS for area in C.AREAS]
    for (limit, area), got in results.items():
        want = C.reference_call(fx, limit, area)
        assert got["gt_overlaps"].dtype == torch.float32 and got["recalls"].dtype == torch.float32
        assert got["gt_overlaps"].numpy().tobytes() == want["gt_overlaps"].tobytes(), (limit, area)
        assert got["num_pos"] == int(want["num_pos"]) > 0
        np.testing.assert_array_equal(got["recalls"].numpy(), want["recalls"])
        np.testing.assert_array_equal(got["thresholds"].numpy(), fx["thresholds"])
        assert abs(float(got["ar"]) - float(want["ar"])) <= AR_TOL


def test_numpy_path_reproduces_the_reference(fx):
    _assert_reference(fx, _evaluate(fx, 12).summarize())


def test_emulated_kernel_reproduces_the_reference(fx, monkeypatch):
    calls = []
    with C.emulated():
        raw = _C.lib.detops_eval_proposal_overlaps
        monkeypatch.setattr(_C.lib, "detops_eval_proposal_overlaps", lambda *a: calls.append(a) or raw(*a), raising=False)
        try:
            ev = _evaluate(fx, 5)
        finally:
            monkeypatch.undo()
    assert len(calls) == 3                                   # one launch per batch, for all 4 x 8 (limit, area) pairs
    _assert_reference(fx, ev.summarize())


def test_batches_of_one_three_and_all_give_identical_results(fx):
    whole = _evaluate(fx, 12).summarize()
    for batch in (1, 3):
        ev = _evaluate(fx, batch)
        assert (ev.num_images, ev.num_detections, ev.num_groundtruths) == (12, int(fx["pred_counts"].sum()), int(fx["gt_counts"].sum()))
        for key, got in ev.summarize().items():
            assert got["gt_overlaps"].numpy().tobytes() == whole[key]["gt_overlaps"].numpy().tobytes()
            assert got["num_pos"] == whole[key]["num_pos"] and torch.equal(got["recalls"], whole[key]["recalls"])
            assert got["ar"].item() == whole[key]["ar"].item()


@pytest.mark.parametrize("limit,area", [(None, "all"), (3, "medium"), (100, "96-128"), (1000, "512-inf")])
def test_evaluate_box_proposals_returns_the_reference_dict(fx, limit, area):
    got = BP.evaluate_box_proposals(C.fixture_predictions(fx), C.FixtureDataset(fx), area=area, limit=limit)
    want = C.reference_call(fx, limit, area)
    assert sorted(got) == ["ar", "gt_overlaps", "num_pos", "recalls", "thresholds"]
    assert got["gt_overlaps"].numpy().tobytes() == want["gt_overlaps"].tobytes() and got["num_pos"] == int(want["num_pos"])
    np.testing.assert_array_equal(got["recalls"].numpy(), want["recalls"])
    assert abs(got["ar"].item() - float(want["ar"])) <= AR_TOL
    # thresholds of the caller's: recalls take their shape and dtype
    own = BP.evaluate_box_proposals(C.fixture_predictions(fx), C.FixtureDataset(fx), thresholds=torch.tensor([0.5, 0.75]),
                                    area=area, limit=limit)
    assert own["recalls"].shape == (2,) and own["recalls"][0] == got["recalls"][0] and own["recalls"][1] == got["recalls"][5]
    with pytest.raises(AssertionError, match="Unknown area range"):
        BP.evaluate_box_proposals([], C.FixtureDataset(fx), area="tiny")


@pytest.mark.parametrize("emulated", [False, True], ids=["numpy", "emulated-kernel"])
def test_operator_against_the_literal_loops(emulated):
    tie, want = C.tie_problem()
    problems = [C.random_problem(11, [(9, 4), (0, 3), (5, 0), (3, 7), (70, 5)]), C.random_problem(12, [(1, 1)], limits=(1,), A=1),
                C.nested_problem(12, 14), tie]
    with (C.emulated() if emulated else contextlib.nullcontext()):
        for pb in problems:
            got = C.run_op(pb)
            assert got.dtype == np.float32 and got.tobytes() == C.literal_overlaps(pb).tobytes()
        assert C.run_op(tie)[0, 0].tobytes() == want.tobytes()


def test_emulated_kernel_against_numpy_at_the_kernels_edges():
    shapes = [(0, 3), (1, 1), (63, 64), (64, 65), (65, 1), (257, 4), (5, 0), (0, 0), (3, 65)]
    for pb in (C.random_problem(21, shapes, limits=(0, 64, 300, 3)), C.nested_problem()):
        want = C.run_op(pb)
        with C.emulated():
            got = C.run_op(pb)
        assert got.tobytes() == want.tobytes()
    assert (want[0, 0] > 0).all() and (want[1, 0] > 0).sum() == 7         # nested: every ground truth reached; limit 7: seven


def test_num_pos_zero_gives_minus_one(fx):
    ev = BP.BoxProposalEvaluator((100,), ("all", "small"))
    t = BoxList(torch.tensor([[10.0, 10.0, 50.0, 60.0]]), (100, 100))
    t.add_field("area", torch.tensor([5000.0]))
    p = BoxList(torch.tensor([[12.0, 10.0, 50.0, 60.0]]), (100, 100))
    p.add_field("objectness", torch.tensor([0.5]))
    ev.update([p], [t])
    ev.update([p], [BoxList(torch.zeros((0, 4)), (100, 100))])             # an image without ground truth
    res = ev.summarize()
    assert res[(100, "small")]["num_pos"] == 0 and res[(100, "small")]["ar"].item() == -1.0
    assert bool((res[(100, "small")]["recalls"] == -1).all()) and res[(100, "small")]["gt_overlaps"].numel() == 0
    assert res[(100, "all")]["num_pos"] == 1 and res[(100, "all")]["ar"].item() == 1.0
    assert BP.BoxProposalEvaluator().summarize()[(1000, "large")]["ar"].item() == -1.0          # nothing fed at all


def test_what_counts_crowds_areas_resize_and_objectness_order():
    t = BoxList(torch.tensor([[10.0, 10.0, 29.0, 29.0], [40.0, 40.0, 59.0, 59.0], [70.0, 10.0, 89.0, 29.0]]), (100, 100))
    t.add_field("iscrowd", torch.tensor([0, 1, 0]))
    t.add_field("area", torch.tensor([1024.0, 1024.0, 9216.0]))            # 32^2: small AND medium; 96^2: medium AND large
    p = BoxList(torch.tensor([[140.0, 5.0, 178.0, 14.5], [20.0, 5.0, 58.0, 14.5]]), (200, 50))       # resized by (0.5, 2)
    p.add_field("objectness", torch.tensor([0.1, 0.9]))
    ev = BP.BoxProposalEvaluator((1, None), ("small", "medium", "large"))
    ev.update([p], [t])
    res = ev.summarize()
    assert [res[(None, a)]["num_pos"] for a in ("small", "medium", "large")] == [1, 2, 1]
    assert res[(None, "medium")]["gt_overlaps"].tolist() == [1.0, 1.0]
    assert res[(1, "medium")]["gt_overlaps"].tolist() == [0.0, 1.0]        # the proposal of objectness 0.9 is the first
    assert res[(1, "small")]["gt_overlaps"].tolist() == [1.0] and res[(1, "large")]["gt_overlaps"].tolist() == [0.0]
    q = BoxList(p.bbox, p.size)
    q.add_field("scores", torch.tensor([0.1, 0.9]))
    with pytest.raises(ValueError, match="not RPN-only"):
        BP.BoxProposalEvaluator().update([q], [t])


def test_generic_entry_points_still_refuse_box_only_and_name_the_way_in(fx):
    from maskrcnn_benchmark.data.synthetic import SyntheticCOCODataset

    ds = SyntheticCOCODataset(2, height=64, width=64, seed=1)
    for call in (lambda: E.evaluate(ds, [], None, box_only=True, iou_types=("bbox",)), lambda: E.check_scope(True, ("bbox",)),
                 lambda: E.coco_evaluation(ds, [], None, box_only=True)):
        with pytest.raises(NotImplementedError, match="box_only") as info:
            call()
        for name in ("inference(box_only=True)", "BoxProposalEvaluator", "evaluate_box_proposals"):
            assert name in str(info.value)
    assert "box_only" in E.__doc__ and "Not built" in E.__doc__


def test_entry_point_argument_checks():
    f = C.emu_proposals_lib().detops_eval_proposal_overlaps
    pb = C.random_problem(5, [(4, 3)], limits=(0,), A=1)
    keep = {k: np.ascontiguousarray(v) for k, v in pb.items()}
    out = np.full((1, 1, 3), -7.0, np.float32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def call(N=1, L=1, A=1, D=4, G=3, max_dt=4, max_gt=3, null=()):
        args = [None if k in null else ptr(keep[k]) for k in ("dt_boxes", "gt_boxes", "dt_offset", "gt_offset", "gt_valid", "limits")]
        return f(*args, N, L, A, D, G, max_dt, max_gt, None if "overlaps" in null else ptr(out), None)

    EINVAL, EUNSUPPORTED = -1, -3
    for bad in (dict(N=-1), dict(L=0), dict(A=0), dict(D=-1), dict(G=-1), dict(max_dt=-1), dict(max_gt=-1), dict(null=("dt_boxes",)),
                dict(null=("gt_boxes",)), dict(null=("dt_offset",)), dict(null=("gt_offset",)), dict(null=("gt_valid",)),
                dict(null=("limits",)), dict(null=("overlaps",)), dict(N=1 << 20, L=1 << 10, A=2)):
        assert call(**bad) == EINVAL, bad
    assert call(max_dt=_abi.EVAL_PROPOSALS_MAX_DT + 1) == EUNSUPPORTED and call(max_gt=_abi.EVAL_PROPOSALS_MAX_GT + 1) == EUNSUPPORTED
    assert call(N=0) == 0 and call(G=0, null=("gt_boxes", "gt_valid", "overlaps")) == 0
    assert (out == -7.0).all()                               # nothing launched so far
    assert call() == 0 and out.tobytes() == C.run_op(pb).tobytes()
    assert _abi.EVAL_PROPOSALS_MAX_DT >= 2048 and _abi.EVAL_PROPOSALS_MAX_GT >= 1024
    assert (_C.EVAL_PROPOSALS_MAX_DT, _C.EVAL_PROPOSALS_MAX_GT) == (_abi.EVAL_PROPOSALS_MAX_DT, _abi.EVAL_PROPOSALS_MAX_GT)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "detops.h")).read()
    assert "#define DETOPS_EVAL_PROPOSALS_MAX_DT %d\n" % _abi.EVAL_PROPOSALS_MAX_DT in header
    assert "#define DETOPS_EVAL_PROPOSALS_MAX_GT %d\n" % _abi.EVAL_PROPOSALS_MAX_GT in header


def test_beyond_the_caps_the_wrapper_takes_the_host_path(monkeypatch):
    pb = C.random_problem(31, [(6, 3), (9, 2)], limits=(0, 4))
    want = C.run_op(pb)
    with C.emulated():
        monkeypatch.setattr(_C, "EVAL_PROPOSALS_MAX_DT", 8)
        called = []
        raw = _C.lib.detops_eval_proposal_overlaps
        monkeypatch.setattr(_C.lib, "detops_eval_proposal_overlaps", lambda *a: called.append(1) or raw(*a), raising=False)
        try:
            assert C.run_op(pb).tobytes() == want.tobytes() and not called           # 9 proposals take part under limit 0
            pb["limits"] = np.array([4, 8], np.int32)
            assert C.run_op(pb).shape == (2, 3, 5) and called                         # at most 8 take part: the kernel
            monkeypatch.setattr(_C, "EVAL_PROPOSALS_MAX_GT", 2)
            del called[:]
            C.run_op(pb)
            assert not called
        finally:
            monkeypatch.undo()


# ------------------------------------------------------------------------------------------------ the model and the tool
TINY = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.RES2_OUT_CHANNELS", "16", "MODEL.RESNETS.WIDTH_PER_GROUP", "4",
        "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", "16", "MODEL.RPN.PRE_NMS_TOP_N_TEST", "100", "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", "50",
        "INPUT.MIN_SIZE_TEST", "96", "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2", "DATALOADER.NUM_WORKERS", "0",
        "DATALOADER.SIZE_DIVISIBILITY", "32"]
KEYS = ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]


def test_inference_box_only_on_an_rpn_only_model(tmp_path):
    from maskrcnn_benchmark.data import make_data_loader
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.engine.inference import inference
    from maskrcnn_benchmark.modeling.detector import build_detection_model

    cfg = load_cfg("rpn_R_50_FPN_1x.yaml", TINY)
    assert cfg.MODEL.RPN_ONLY and cfg.MODEL.RPN.USE_FPN and cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST == 50
    torch.manual_seed(0)
    folder = str(tmp_path / "out")
    with cpu_shim.install():
        model = build_detection_model(cfg)
        res = inference(model, make_data_loader(cfg, is_train=False, length=4), "synthetic", box_only=True, device="cpu",
                        output_folder=folder)
        assert list(res.results) == ["box_proposal"] and list(res.results["box_proposal"]) == KEYS
        values = list(res.results["box_proposal"].values())
        assert all(v == -1 or 0.0 <= v <= 1.0 for v in values) and 0.0 <= values[0] <= 1.0 and 0.0 <= values[4] <= 1.0
        assert sorted(os.listdir(folder)) == ["box_proposals.pth", "box_proposals.txt"]          # no result files for proposals
        assert "Task: box_proposal" in open(os.path.join(folder, "box_proposals.txt")).read()
        saved = torch.load(os.path.join(folder, "box_proposals.pth"), weights_only=False)
        assert saved.results == res.results
        # what stays refused
        loader = make_data_loader(cfg, is_train=False, length=2)
        with pytest.raises(NotImplementedError, match="box_only"):
            inference(model, loader, "synthetic", box_only=True, device="cpu", keypoint_oks=True)
        with pytest.raises(NotImplementedError, match="box_only"):
            inference(model, loader, "synthetic", box_only=True, device="cpu", evaluate=False, output_folder=folder)
        with pytest.raises(NotImplementedError, match="box_only"):
            inference(model, loader, "synthetic", box_only=True, device="cpu", bbox_aug=True, cfg=cfg)


def test_inference_box_only_refuses_a_model_that_is_not_rpn_only():
    from maskrcnn_benchmark.data.synthetic import BatchCollator, SyntheticCOCODataset
    from maskrcnn_benchmark.engine.inference import inference

    dataset = SyntheticCOCODataset(2, height=64, width=64, seed=3)

    class Detector(torch.nn.Module):
        def forward(self, images):
            out = []
            for _ in range(images.tensors.shape[0]):
                b = BoxList(torch.tensor([[1.0, 2.0, 30.0, 40.0]]), (64, 64))
                b.add_field("scores", torch.tensor([0.5]))
                b.add_field("labels", torch.tensor([1]))
                out.append(b)
            return out

    loader = torch.utils.data.DataLoader(dataset, batch_size=2, shuffle=False, num_workers=0, collate_fn=BatchCollator(0))
    with pytest.raises(ValueError, match="not RPN-only"):
        inference(Detector(), loader, "synthetic", box_only=True, device="cpu")


def test_test_net_prints_the_proposal_table_and_the_config_still_trains(tmp_path, capsys):
    import test_net
    from maskrcnn_benchmark.data import make_data_loader
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model

    torch.manual_seed(0)
    with cpu_shim.install():
        res = test_net.main(["--config-file", "rpn_R_50_FPN_1x.yaml", "--images", "4"] + TINY + ["OUTPUT_DIR", str(tmp_path / "run")])
    printed = capsys.readouterr().out
    assert "Task: box_proposal" in printed and ", ".join(KEYS) in printed
    assert list(res[0].results["box_proposal"]) == KEYS
    assert sorted(os.listdir(tmp_path / "run" / "inference" / "synthetic_coco_val")) == ["box_proposals.pth", "box_proposals.txt"]
    cfg = load_cfg("rpn_R_50_FPN_1x.yaml", TINY)
    with cpu_shim.install():
        model = build_detection_model(cfg).train()
        images, targets, _ = next(iter(make_data_loader(cfg, is_train=False, length=2)))
        losses = model(images, targets)
        assert sorted(losses) == ["loss_objectness", "loss_rpn_box_reg"]
        sum(losses.values()).backward()
        assert all(torch.isfinite(v) for v in losses.values())
