"""The edge cases of tests/pool_edge_cases.py on the host: csrc/roi_pool.hip, csrc/deform_pool.hip and csrc/f64_ops.hip.

Two things per case.  First the oracle is pinned to an independent reference at the new edges, so that the device test may
trust it there: ROIPool to the plain loop `torch_refs.roi_pool_py`, deformable PS-ROI pooling to the fp64 autograd
formulation `torch_refs.deform_psroi_pool_torch` (written from the operator's definition), ROIAlign to
`torch_refs.roi_align_torch` in fp64, the focal loss to the fp64 formula of tests/golden/make_golden_focal_formula.py, NMS to
the greedy loop of the case module.  Then the same case runs through the host emulation of the kernels (tests/emu: the same
HIP sources, workgroups one after another) behind the product's own `_C` wrappers, with exactly the assertions
tests/test_pool_edges_gpu.py makes on the device."""
import numpy as np
import pytest
import torch

import cpu_shim
import oracle
import pool_edge_cases as pc
from torch_refs import deform_psroi_pool_torch, roi_pool_py


@pytest.fixture
def ops():
    with cpu_shim.install("emu-lib"):
        yield pc.Ops("cpu")


# ------------------------------------------------------------------------------------------ ROIPool, fp32
@pytest.mark.parametrize("name", pc.ROI_POOL_CASES)
def test_oracle_roi_pool_equals_the_plain_loop(name):
    c = pc.roi_pool_case(name)
    for (PH, PW), e in zip(c["pools"], pc.roi_pool_expected(name)):
        out, amax = roi_pool_py(c["x"], c["rois"], c["scale"], PH, PW)
        assert np.array_equal(amax, e["amax"]) and pc.same_bits(out, e["out"]), (name, PH, PW)
        # the backward from its definition: every bin adds its gradient at its argmax (integers: exact in any order)
        want = np.zeros(c["x"].shape, np.float64)
        K, C = amax.shape[:2]
        for k in range(K):
            plane = want[int(c["rois"][k, 0])].reshape(C, -1)
            for ch in range(C):
                a = amax[k, ch].ravel()
                np.add.at(plane[ch], a[a >= 0], e["g"][k, ch].ravel()[a >= 0])
        assert pc.same_bits(e["gin"], want.astype(np.float32)), (name, PH, PW)
    pc.roi_pool_case_properties(name)


@pytest.mark.parametrize("name", pc.ROI_POOL_CASES)
def test_emu_roi_pool_edge_cases(ops, name):
    pc.check_roi_pool(ops, name)


def test_emu_roi_pool_backward_accumulates(ops):
    pc.check_roi_pool_accumulate(ops)


@pytest.mark.parametrize("name", sorted(pc.PLANE_FORM))
def test_emu_roi_pool_backward_form_by_plane_size(ops, name):
    pc.check_roi_pool_form(ops, name)


# ------------------------------------------------------------------------------------------ deformable PS-ROI pooling
@pytest.mark.parametrize("name", sorted(pc.PSROI_CASES))
def test_oracle_psroi_equals_the_autograd_formulation(name):
    c, cfg, e = pc.psroi_case(name), pc.psroi_cfg(name), pc.psroi_expected(name)
    x = torch.tensor(c["data"]).double().requires_grad_(True)
    t = None if c["trans"] is None else torch.tensor(c["trans"]).double().requires_grad_(True)
    y, cnt = deform_psroi_pool_torch(x, torch.tensor(c["rois"]).double(), t, *cfg)
    assert np.array_equal(e["cnt"], cnt.numpy().astype(np.float32)), name
    np.testing.assert_allclose(e["out"], y.detach().numpy(), rtol=1e-4, atol=1e-5)
    y.backward(torch.tensor(e["g"]).double())
    np.testing.assert_allclose(e["gin"], x.grad.numpy(), rtol=1e-4, atol=1e-4)
    if t is not None:
        tref = t.grad.numpy()
        np.testing.assert_allclose(e["gtr"], tref, rtol=1e-3, atol=1e-3 * max(1.0, float(np.abs(tref).max())))


@pytest.mark.parametrize("name", sorted(pc.PSROI_CASES))
def test_emu_psroi_edge_cases(ops, name):
    pc.check_psroi(ops, name)


def test_emu_psroi_backward_accumulates(ops):
    pc.check_psroi_accumulate(ops)


def test_emu_psroi_refusals_write_nothing(ops):
    pc.check_psroi_refusals(ops)


# ------------------------------------------------------------------------------------------ fp64 operators
@pytest.mark.parametrize("cfg", pc.ALIGN64_CFGS)
def test_oracle_roi_align_near_the_fp64_formulation(cfg):
    """the fp32 oracle against roi_align_torch in fp64: a bin sums 4 taps of gh x gw samples in fp32, each product rounded
    once and the running sum once per term: |error| <= 2 (4 gh gw + 1) 2^-24 max|x| per bin before the division"""
    c = pc.align64_case()
    PH, PW, sr = cfg
    x32, r32 = c["x"].astype(np.float32), c["rois"].astype(np.float32)
    want, _ = pc.align64_reference(x32.astype(np.float64), r32.astype(np.float64), c["scale"], PH, PW, sr)
    got = oracle.roi_align_forward(x32, r32, c["scale"], PH, PW, sr)
    side = np.maximum((r32[:, 3:] - r32[:, 1:3]) * c["scale"], 1.0)
    grid = sr * sr if sr > 0 else np.ceil(side[:, 0] / PW) * np.ceil(side[:, 1] / PH)
    bound = 2 * (4 * grid + 1) * 2.0 ** -24 * np.abs(x32).max()
    assert (np.abs(got - want).max((1, 2, 3)) <= bound).all()


@pytest.mark.parametrize("cfg", pc.ALIGN64_CFGS)
def test_emu_roi_align_f64_edge_rois(ops, cfg):
    pc.check_align64(ops, cfg)


def test_oracle_roi_align_contains_non_finite_pixels():
    c = pc.align_containment_case()
    x32, clean32, r32 = c["x"].astype(np.float32), c["clean"].astype(np.float32), c["rois"].astype(np.float32)
    for PH, PW, sr in c["cfgs"]:
        dirty = oracle.roi_align_forward(x32, r32, c["scale"], PH, PW, sr)
        assert np.isfinite(dirty).all() and pc.same_bits(dirty, oracle.roi_align_forward(clean32, r32, c["scale"], PH, PW, sr))
        a, _ = pc.align64_reference(c["x"], c["rois"], c["scale"], PH, PW, sr)
        b, _ = pc.align64_reference(c["clean"], c["rois"], c["scale"], PH, PW, sr)
        assert np.isfinite(a).all() and np.abs(a - b).max() <= 1e-12 and np.abs(dirty - b).max() <= 1e-5


def test_emu_roi_align_f64_contains_non_finite_pixels(ops):
    pc.check_align_containment_f64(ops)


def test_emu_roi_align_f32_contains_non_finite_pixels(ops):
    pc.check_align_containment_f32(ops)


@pytest.mark.parametrize("name", ("ties", "windows", "non_finite"))
def test_emu_roi_pool_f64_equals_the_fp32_oracle(ops, name):
    pc.check_roi_pool_f64(ops, name)


def test_emu_roi_pool_f64_window_below_flt_max(ops):
    pc.check_roi_pool_f64_below_flt_max(ops)


@pytest.mark.parametrize("C,gamma", pc.FOCAL_CASES)
def test_oracle_focal_near_the_fp64_formula(C, gamma):
    c = pc.focal_case(C, gamma)
    f = oracle.sigmoid_focal_loss_forward(c["logits"], c["targets"], gamma, pc.FOCAL_ALPHA)
    b = oracle.sigmoid_focal_loss_backward(c["logits"], c["targets"], c["d"], gamma, pc.FOCAL_ALPHA)
    np.testing.assert_allclose(f, c["loss"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(b, c["grad"], rtol=1e-4, atol=1e-6)
    ign = c["targets"] < 0
    assert not f[ign].any() and not b[ign].any() and not c["loss"][ign].any() and not c["grad"][ign].any()


@pytest.mark.parametrize("C,gamma", pc.FOCAL_CASES)
def test_emu_focal_f64_extreme_logits(ops, C, gamma):
    pc.check_focal_f64(ops, C, gamma)


@pytest.mark.parametrize("name", pc.NMS64_CASES)
def test_oracle_nms_equals_the_greedy_loop_in_fp32(name):
    """the fp32 oracle agrees with the greedy loop evaluated in fp32 (for the case below fp32 resolution: the other set)"""
    c = pc.nms64_case(name)
    assert np.array_equal(oracle.nms(c["boxes"], c["scores"], c["thr"]), pc.nms_greedy(c["boxes"], c["scores"], c["thr"], np.float32))


@pytest.mark.parametrize("name", pc.NMS64_CASES)
def test_emu_nms_f64_words_ties_and_resolution(ops, name):
    pc.check_nms64(ops, name)
