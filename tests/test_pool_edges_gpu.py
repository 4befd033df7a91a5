"""The edge cases of tests/pool_edge_cases.py on the device through maskrcnn_benchmark._C (and the C ABI under it where a
flag has no `_C` spelling): csrc/roi_pool.hip, csrc/deform_pool.hip and csrc/f64_ops.hip where small, odd and non-finite
inputs take them — tied maxima, windows off the map, -inf / NaN planes, the window computation without the LDS table, three
rounds of the plane owner's ROI list, planes around its LDS limit, accumulation into the caller's gradients; offset gradients
through global atomics, the table-less sampling path, bins wider than a thread's private window, one-row and one-column
maps, samples on pixel centres and on the inclusive limits, the refusal codes; fp64 ROIAlign with samples on and beyond the
limits and non-finite pixels next to them, fp64 ROIPool below -FLT_MAX, fp64 focal loss at |x| = 100, fp64 NMS across mask
words and below fp32 resolution.  tests/test_pool_edges_emu.py holds the same checks on the host emulation, after pinning
the oracle to independent references on every case.

Bit equality where the operation is exact (ROIPool forward, argmax, its backward on integer gradients in every form, sample
counts, kept sets); elsewhere the tolerances of tests/test_ops_gpu.py for the same operators."""
import pytest

import pool_edge_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return pc.Ops("cuda")


# ------------------------------------------------------------------------------------------ ROIPool, fp32
@pytest.mark.parametrize("name", pc.ROI_POOL_CASES)
def test_roi_pool_edge_cases(ops, name):
    pc.roi_pool_case_properties(name)
    pc.check_roi_pool(ops, name)


def test_roi_pool_backward_accumulates(ops):
    pc.check_roi_pool_accumulate(ops)


@pytest.mark.parametrize("name", sorted(pc.PLANE_FORM))
def test_roi_pool_backward_form_by_plane_size(ops, name):
    pc.check_roi_pool_form(ops, name)


# ------------------------------------------------------------------------------------------ deformable PS-ROI pooling
@pytest.mark.parametrize("name", sorted(pc.PSROI_CASES))
def test_psroi_edge_cases(ops, name):
    pc.check_psroi(ops, name)


def test_psroi_backward_accumulates(ops):
    pc.check_psroi_accumulate(ops)


def test_psroi_refusals_write_nothing(ops):
    pc.check_psroi_refusals(ops)


# ------------------------------------------------------------------------------------------ fp64 operators
@pytest.mark.parametrize("cfg", pc.ALIGN64_CFGS)
def test_roi_align_f64_edge_rois(ops, cfg):
    pc.check_align64(ops, cfg)


def test_roi_align_f64_contains_non_finite_pixels(ops):
    pc.check_align_containment_f64(ops)


def test_roi_align_f32_contains_non_finite_pixels(ops):
    pc.check_align_containment_f32(ops)


@pytest.mark.parametrize("name", ("ties", "windows", "non_finite"))
def test_roi_pool_f64_equals_the_fp32_oracle(ops, name):
    pc.check_roi_pool_f64(ops, name)


def test_roi_pool_f64_window_below_flt_max(ops):
    pc.check_roi_pool_f64_below_flt_max(ops)


@pytest.mark.parametrize("C,gamma", pc.FOCAL_CASES)
def test_focal_f64_extreme_logits(ops, C, gamma):
    pc.check_focal_f64(ops, C, gamma)


@pytest.mark.parametrize("name", pc.NMS64_CASES)
def test_nms_f64_words_ties_and_resolution(ops, name):
    pc.check_nms64(ops, name)
