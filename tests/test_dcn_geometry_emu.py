"""The check bodies of tests/dcn_geometry_cases.py on CPU tensors through the product's own `_C` wrappers over the host
emulation of the HIP sources (tests/cpu_shim.py, backend "emu-lib"): the cases, the exact-arithmetic inputs and the oracle
are proven here without a GPU; tests/test_dcn_geometry_gpu.py runs the same bodies on the device.  The emulation has no
bf16, so half precision is fp16 here (bf16 runs on the device only)."""
import pytest
import torch

import cpu_shim
import dcn_geometry_cases as G

DEV = "cpu"
HALF = [torch.float16]


@pytest.fixture(autouse=True)
def _product_wrappers():
    with cpu_shim.install("emu-lib"):
        yield
_id = lambda v: v.name if isinstance(v, G.Case) else str(v).replace("torch.", "")  # noqa: E731


@pytest.fixture
def transposed(monkeypatch):
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(_C, "DCN_INPUT_GRAD", "transposed")


# ---------------------------------------------------------------------------------------------- fused MFMA forward
@pytest.mark.parametrize("modulated", [False, True])
@pytest.mark.parametrize("dtype", HALF, ids=_id)
@pytest.mark.parametrize("case", G.FUSED_CASES, ids=_id)
def test_fused_forward_is_bit_equal_to_the_rounded_oracle(case, dtype, modulated):
    G.check_fused_forward(DEV, case, dtype, modulated)


def test_fused_forward_is_chosen_by_the_auto_rule_at_a_res2_sized_half_layer():
    """C = Cout = 64 in fp16 on a 130 x 128 map: no switch set, the counter shows dcn_fused_fwd (BKC = 64), bit-equal"""
    G.check_fused_forward(DEV, G.FUSED_AUTO, torch.float16, True, force=False)


@pytest.mark.parametrize("dtype", HALF, ids=_id)
def test_fused_forward_on_random_floats(dtype):
    G.check_fused_forward(DEV, G.FUSED_CASES[1], dtype, True, kind="float")


# ---------------------------------------------------------------------------------------------- channels-last pipeline, fp32
@pytest.mark.parametrize("case,modulated", G.NHWC_FP32_LAYER_RUNS, ids=G.run_id)
def test_channels_last_pipeline_fp32_is_bit_equal_to_the_oracle(case, modulated):
    G.check_nhwc_layer(DEV, case, torch.float32, modulated)


@pytest.mark.parametrize("modulated", [False, True])
def test_channels_last_pipeline_fp32_on_channels_last_tensors(modulated):
    G.check_nhwc_layer(DEV, G.NHWC_S2D2, torch.float32, modulated, channels_last=True)


@pytest.mark.parametrize("modulated", [False, True])
@pytest.mark.parametrize("case", [G.NHWC_RECT_1X3, G.NHWC_RECT_3X1], ids=_id)
def test_channels_last_reference_names_rectangular(case, modulated):
    G.check_nhwc_reference_names(DEV, case, modulated)


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("case,modulated", [(G.NHWC_S2D2, False), (G.NHWC_S2D2, True), (G.NHWC_RECT_1X3, False)],
                         ids=["s2d2-v1", "s2d2-v2", "rect-1x3-v1"])
def test_transposed_sampling_input_gradient_fp32_is_bit_equal_to_the_oracle(transposed, case, modulated, channels_last):
    G.check_nhwc_layer(DEV, case, torch.float32, modulated, channels_last=channels_last, input_grad="transposed")


@pytest.mark.parametrize("input_grad", ["col2im", "transposed"])
def test_channels_last_pipeline_fp32_on_random_floats(monkeypatch, input_grad):
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(_C, "DCN_INPUT_GRAD", input_grad)
    G.check_nhwc_layer(DEV, G.NHWC_S2D2, torch.float32, True, input_grad=input_grad, kind="float")


# ---------------------------------------------------------------------------------------------- channels-last pipeline, half
@pytest.mark.parametrize("modulated", [False, True])
@pytest.mark.parametrize("dtype", HALF, ids=_id)
def test_channels_last_pipeline_half(dtype, modulated):
    G.check_nhwc_layer(DEV, G.NHWC_S2D2_HALF, dtype, modulated)


@pytest.mark.parametrize("dtype", HALF, ids=_id)
def test_channels_last_pipeline_half_transposed_sampling(transposed, dtype):
    G.check_nhwc_layer(DEV, G.NHWC_S2D2_HALF, dtype, True, input_grad="transposed")


@pytest.mark.parametrize("dtype", HALF, ids=_id)
def test_half_cout_64_is_outside_the_channels_last_plan_and_takes_the_reference_layout_kernels(dtype):
    G.check_nhwc_layer(DEV, G.NHWC_S2D2, dtype, True, in_plan=False)


def test_channels_last_pipeline_fp16_four_vectors_per_lane():
    G.check_nhwc_layer(DEV, G.NHWC_NV4_HALF, torch.float16, True)


@pytest.mark.parametrize("dtype", HALF, ids=_id)
def test_channels_last_pipeline_half_on_random_floats(dtype):
    G.check_nhwc_layer(DEV, G.NHWC_S2D2_HALF, dtype, True, kind="float")


# ---------------------------------------------------------------------------------------------- overflow list
PILE_FP32 = G._c("pile-64", 1, 64, 8, 8, 64, 3, 1, 1, 1)
PILE_FP32_LONG = G._c("pile-64-12x12", 1, 64, 12, 12, 64, 3, 1, 1, 1)
PILE_FP16 = G._c("pile-128", 1, 128, 8, 8, 128, 3, 1, 1, 1)


@pytest.mark.parametrize("case", [PILE_FP32, PILE_FP32_LONG], ids=_id)
@pytest.mark.parametrize("input_grad", ["col2im", "transposed"])
def test_overflow_list_fp32_input_gradient_is_bit_equal_to_the_oracle(monkeypatch, input_grad, case):
    """H * W contributions per (pixel, tap) against 8 slots, the rest through the overflow list.  8 x 8: 4 x 9 x 56 = 2016 entries,
    which the col2im form reduces per pixel in fp32; 12 x 12: 4896 entries, beyond that kernel's limit of 4096, added entry by
    entry with fp32 atomics, which are order-free on exactly representable partial sums (as are those of the transposed form)"""
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(_C, "DCN_INPUT_GRAD", input_grad)
    G.check_overflow(DEV, case, torch.float32, (3.25, 4.5), input_grad)


@pytest.mark.parametrize("input_grad", ["col2im", "transposed"])
@pytest.mark.parametrize("dtype,case,landing", [(torch.float16, PILE_FP16, (3.25, 4.5))], ids=["float16"])
def test_overflow_list_half_input_gradient(monkeypatch, dtype, case, landing, input_grad):
    """the overflow list in fp16 (the emulation's stand-in for the packed atomics rounds every add like the hardware
    instruction): within the project's 2e-2 of max|ref|; the bf16 case and the bounds: tests/test_dcn_geometry_gpu.py"""
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(_C, "DCN_INPUT_GRAD", input_grad)
    G.check_overflow(DEV, case, dtype, landing, input_grad)


# ---------------------------------------------------------------------------------------------- reference-layout kernels
@pytest.mark.parametrize("ell_build", [0, 1])
@pytest.mark.parametrize("col2im", [1, 2, 3])
@pytest.mark.parametrize("case", G.REF_RECT_CASES, ids=_id)
def test_reference_layout_kernels_rectangular_are_bit_equal_to_the_oracle(case, col2im, ell_build):
    G.check_ref_layout_rect(DEV, case, col2im, ell_build)


# ---------------------------------------------------------------------------------------------- 16-bit atomics, ragged transposes
@pytest.mark.parametrize("dtype", HALF, ids=_id)
@pytest.mark.parametrize("case", [G.HALF_ATOMIC, G.HALF_ATOMIC_TALL], ids=_id)
def test_scatter_col2im_half_is_bit_equal_to_the_rounded_oracle(case, dtype):
    G.check_half_atomic_col2im(DEV, case, dtype, 2)


@pytest.mark.parametrize("ell_build", [0, 1])
@pytest.mark.parametrize("dtype", HALF, ids=_id)
def test_ell_overflow_col2im_half_is_bit_equal_to_the_rounded_oracle(dtype, ell_build):
    G.check_half_atomic_col2im(DEV, G.HALF_ATOMIC, dtype, 3, ell_build)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=_id)
def test_to_nhwc_ragged_channel_and_pixel_tiles(dtype):
    G.check_to_nhwc_tails(DEV, dtype)
