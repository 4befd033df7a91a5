"""csrc/eval_proposals.hip on the device: the fixture of the REFERENCE's evaluate_box_proposals
(tests/golden/box_proposals_reference.npz) and the numpy path (_eval_cpu.eval_proposal_overlaps, pinned to the fixture and to
literal loops by tests/test_box_proposals_cpu.py) bit for bit, at the shapes where the kernel can go wrong, and an RPN-only
model through `inference(box_only=True)` against the CPU path on the same proposals.

Every path makes an IoU by the same IEEE fp32 operations in the same order and compares them exactly, so everything here is
compared bit for bit; `ar` against the reference within 10 * 2^-24 (tests/test_box_proposals_cpu.py).
"""
import numpy as np
import pytest
import torch

import box_proposal_cases as C
from maskrcnn_benchmark import _C
from maskrcnn_benchmark.data.datasets import evaluation as E
from maskrcnn_benchmark.data.datasets.evaluation import box_proposals as BP

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_DT, MAX_GT = _C.EVAL_PROPOSALS_MAX_DT, _C.EVAL_PROPOSALS_MAX_GT


def _both(pb):
    """-> the device's result, run twice with equal bits, after comparing it with the numpy path's"""
    got, again, want = C.run_op(pb, DEV), C.run_op(pb, DEV), C.run_op(pb)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == again.tobytes()
    assert got.tobytes() == want.tobytes(), "%d of %d differ" % (int((got != want).sum()), got.size)
    return got


def test_fixture_on_the_device_against_the_reference_and_the_numpy_path():
    fx = C.load_fixture()
    dataset = C.FixtureDataset(fx)
    dev = E._feed(BP.BoxProposalEvaluator(C.LIMITS, C.AREAS), C.fixture_predictions(fx, DEV), dataset, 5, DEV)
    cpu = E._feed(BP.BoxProposalEvaluator(C.LIMITS, C.AREAS), C.fixture_predictions(fx), dataset, 5)
    assert all(o.is_cuda for o, _ in dev.batches) and len(dev.batches) == 3
    for (a, _), (b, _) in zip(dev.batches, cpu.batches):
        assert a.cpu().numpy().tobytes() == b.numpy().tobytes()
    cpu_res = cpu.summarize()
    for (limit, area), got in dev.summarize().items():
        want = C.reference_call(fx, limit, area)
        assert got["gt_overlaps"].numpy().tobytes() == want["gt_overlaps"].tobytes(), (limit, area)
        assert got["num_pos"] == int(want["num_pos"])
        np.testing.assert_array_equal(got["recalls"].numpy(), want["recalls"])
        assert abs(got["ar"].item() - float(want["ar"])) <= 10 * 2.0 ** -24
        assert got["ar"].item() == cpu_res[(limit, area)]["ar"].item()


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 257])
def test_proposal_counts_across_wave_and_workgroup_edges(P):
    # G in {0, 1, 64, 65} beside every P (G' > P' and P' > G' both occur); limits below, at and above P and none; the last
    # area range counts no ground truth; images without proposals or ground truth between full ones
    shapes = [(P, 0), (P, 1), (0, 2), (P, 64), (0, 0), (P, 65), (3, 0), (P, 5)]
    got = _both(C.random_problem(100 + P, shapes, limits=(max(P - 1, 1), P, P + 1, 0)))
    assert (got[:, -1] == -1).all() and (got[:, 0] >= 0).all()


def test_every_round_scans_every_column_again_and_the_built_ties():
    got = _both(C.nested_problem())                     # 65 ground truths that all prefer proposal 0, then 1, ...
    assert (got[0, 0] > 0).all() and (got[1, 0] > 0).sum() == 7
    tie, want = C.tie_problem()
    assert _both(tie)[0, 0].tobytes() == want.tobytes()


def test_at_each_cap_and_one_above(monkeypatch):
    at = C.random_problem(7, [(MAX_DT, 3), (5, MAX_GT), (0, 1)], limits=(0, MAX_DT), A=2)
    calls = []
    raw = _C.lib.detops_eval_proposal_overlaps
    monkeypatch.setattr(_C.lib, "detops_eval_proposal_overlaps", lambda *a: calls.append(1) or raw(*a), raising=False)
    try:
        got = _both(at)
        assert len(calls) == 2 and got.shape == (2, 2, 3 + MAX_GT + 1)
        # one proposal more takes part only without a limit: the limited call still goes to the kernel
        over = C.random_problem(8, [(MAX_DT + 1, 3)], limits=(MAX_DT,), A=1)
        _both(over)
        assert len(calls) == 4
        over["limits"] = np.array([0], np.int32)
        assert C.run_op(over, DEV).tobytes() == C.run_op(over).tobytes() and len(calls) == 4       # the host path
        over = C.random_problem(9, [(5, MAX_GT + 1)], limits=(0,), A=1)
        assert C.run_op(over, DEV).tobytes() == C.run_op(over).tobytes() and len(calls) == 4
    finally:
        monkeypatch.undo()


def test_guards_stay_untouched_and_the_entry_point_refuses_without_launching():
    guard = 16
    pb = C.random_problem(13, [(70, 5), (0, 3), (9, 66)], limits=(0, 8), A=2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    args = [t(pb[k]) for k in ("dt_boxes", "gt_boxes", "dt_offset", "gt_offset", "gt_valid", "limits")]
    G_total = pb["gt_boxes"].shape[0]
    out = torch.full((2 * 2 * G_total + 2 * guard,), -7.0, dtype=torch.float32, device=DEV)

    def call(max_dt=70, max_gt=66, L=2):
        rc = _C.lib.detops_eval_proposal_overlaps(*(a.data_ptr() for a in args), 3, L, 2, pb["dt_boxes"].shape[0], G_total, max_dt, max_gt,
                                                  out.data_ptr() + 4 * guard, _C.stream_of(out))
        torch.cuda.synchronize()
        return rc

    for kw, code in ((dict(max_dt=MAX_DT + 1), -3), (dict(max_gt=MAX_GT + 1), -3), (dict(L=0), -1), (dict(max_dt=-1), -1)):
        assert call(**kw) == code
        assert bool((out == -7.0).all())
    assert call() == 0
    got = out.cpu().numpy()
    assert (got[:guard] == -7.0).all() and (got[-guard:] == -7.0).all()
    assert got[guard:-guard].tobytes() == C.run_op(pb).tobytes()


# ------------------------------------------------------------------------------------------------ the model
TINY = ["MODEL.RESNETS.RES2_OUT_CHANNELS", "16", "MODEL.RESNETS.WIDTH_PER_GROUP", "4", "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", "16",
        "MODEL.RPN.PRE_NMS_TOP_N_TEST", "200", "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", "150", "INPUT.MIN_SIZE_TEST", "96",
        "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2", "DATALOADER.NUM_WORKERS", "0", "DATALOADER.SIZE_DIVISIBILITY", "32"]


class _Recorded(torch.nn.Module):
    """the model, keeping a CPU copy of what it returned"""

    def __init__(self, model):
        super().__init__()
        self.model, self.outputs = model, []

    def forward(self, images):
        out = self.model(images)
        self.outputs += [o.to("cpu") for o in out]
        return out


@pytest.mark.parametrize("layout", ["all", "nchw"], ids=["channels-last", "nchw"])
def test_rpn_only_model_through_inference_gives_the_cpu_paths_table(layout, monkeypatch):
    from maskrcnn_benchmark.data import make_data_loader
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.engine.inference import inference
    from maskrcnn_benchmark.modeling.detector import build_detection_model

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    cfg = load_cfg("rpn_R_50_FPN_1x.yaml", TINY)
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(DEV)
    if layout != "nchw":
        model.set_channels_last(True, heads=True)
    recorded = _Recorded(model)
    loader = make_data_loader(cfg, is_train=False, length=4)
    res = inference(recorded, loader, "synthetic", box_only=True, device=DEV)
    row = res.results["box_proposal"]
    assert list(row) == ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]
    assert len(recorded.outputs) == 4 and all(o.has_field("objectness") for o in recorded.outputs)
    print("%s: proposals per image %s, %s" % (layout, [len(o) for o in recorded.outputs], dict(row)))
    cpu = E.do_box_proposal_evaluation(loader.dataset, recorded.outputs)
    assert cpu.results["box_proposal"] == row
    assert 0.0 <= row["AR@100"] <= 1.0 and 0.0 <= row["AR@1000"] <= 1.0
