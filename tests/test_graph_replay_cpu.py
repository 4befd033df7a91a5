"""The pure helpers of tests/graph_replay.py (bit views, poison patterns, replay order) on the host."""
import numpy as np
import pytest
import torch

import graph_replay as gr


def test_bit_views_tell_what_value_comparison_hides():
    nan = torch.tensor([float("nan"), 1.0, -0.0])
    assert not torch.equal(nan, nan.clone()) and gr.bits_equal(nan, nan.clone())          # NaN equals NaN
    assert torch.equal(torch.tensor([0.0]), torch.tensor([-0.0])) and not gr.bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    other_nan = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)         # another payload
    assert other_nan.isnan().all() and not gr.bits_equal(other_nan, torch.tensor([float("nan")]))
    for dt, width in ((torch.float64, torch.int64), (torch.float32, torch.int32), (torch.float16, torch.int16),
                      (torch.bfloat16, torch.int16), (torch.bool, torch.uint8), (torch.int64, torch.int64), (torch.uint8, torch.uint8)):
        t = torch.ones(2, 3).to(dt)
        assert gr.bit_view(t).dtype == width and gr.bit_view(t).shape == t.shape
    # same values, different dtype or shape: not equal
    assert not gr.bits_equal(torch.zeros(4), torch.zeros(4, dtype=torch.float64))
    assert not gr.bits_equal(torch.zeros(4), torch.zeros(2, 2))
    assert gr.bits_equal(np.arange(4, dtype=np.int64), torch.arange(4))
    # a channels-last tensor is compared in index order, not storage order
    a = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).view(2, 3, 4, 5)
    assert gr.bits_equal(a, a.contiguous(memory_format=torch.channels_last))


def test_first_difference_names_the_element():
    a, b = torch.zeros(2, 3), torch.zeros(2, 3)
    assert gr.first_difference(a, b) == "equal"
    b[1, 2] = 5
    assert "1 of 6" in gr.first_difference(a, b) and "(1, 2)" in gr.first_difference(a, b)
    assert "float64" in gr.first_difference(a, b.double())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int64, torch.int32,
                                   torch.uint8, torch.bool])
def test_poison_is_a_pattern_no_result_holds(dtype):
    t = torch.zeros(3, 5).to(dtype)
    assert not gr.is_poison(t)
    gr.poison_(t)
    assert gr.is_poison(t)
    if dtype.is_floating_point:
        assert bool(t.isnan().all())
    elif dtype == torch.bool:
        assert bool((t.view(torch.uint8) == 0xFF).all())           # neither False (0) nor True (1)
        assert not gr.bits_equal(t, torch.ones(3, 5, dtype=torch.bool))
    elif dtype == torch.uint8:
        assert bool((t == 0xFF).all())
    else:
        assert bool((t == -1).all())
    t.view(-1)[0:1].copy_(torch.zeros(1).to(dtype))                 # one element written: no longer "all poison"
    assert not gr.is_poison(t)
    assert not gr.is_poison(torch.zeros(0).to(dtype))


def test_assert_bits_reports_count_none_and_position():
    x = torch.tensor([1.0, 2.0])
    gr.assert_bits((x, None), (x.clone(), None), "same")
    gr.assert_bits(x, x.clone(), "a single tensor is a tuple of one")
    with pytest.raises(AssertionError, match="2 outputs vs 1"):
        gr.assert_bits((x, x), (x,), "count")
    with pytest.raises(AssertionError, match="None on one side"):
        gr.assert_bits((x, None), (x, x), "none")
    with pytest.raises(AssertionError, match="output 1"):
        gr.assert_bits((x, x), (x, torch.tensor([1.0, 3.0])), "value")
    with pytest.raises(AssertionError):
        gr.assert_bits(gr.poison_(x.clone()), x, "poison left in an output")


def test_replay_order_ends_on_the_first_set_twice_the_last_time_without_reload():
    assert gr.replay_order(3) == [(0, True), (1, True), (2, True), (0, True), (0, False)]
    assert gr.replay_order(1) == [(0, True), (0, True), (0, False)]
