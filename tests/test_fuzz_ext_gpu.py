"""The extension-operator families of tests/fuzz_cases.py (`fuzz_cases.EXTENSION`) on the MI355X — run with `-m gpu`.  The device
sibling of tests/test_emu_fuzz_ext.py: same families, same seeds, the same cases bit for bit
(tests/golden/fuzz_case_digests.json), the same calls and references (tests/fuzz_ext_runs.py).

These are the operators the project added beyond the reference's `_C` — csrc/targets.hip, head_loss.hip, keypoint.hip,
masker.hip, rle_string.hip, rle_decode.hip, evaluate.hip, bbox_aug.hip, group_norm.hip, bias_act.hip — and the ones that lean
hardest on workspaces and on state handed from one launch to the next (count / host read / write pairs, the three launches of
the keypoint loss, the four of mask_pack_rle, the device-side row lists of the sparse RPN-head backward).  Every workspace is
cut from `torch.empty` inside `_C`, so every case runs twice in the same test (tests/dirty_memory.py::_clean_then_dirty): once
on the allocator as it is, once after 0xFF bytes — NaN in every float type, -1 in every integer type — were left in the free
blocks that the next allocations are cut from.  Both runs meet the reference.  Everything include/detops.h calls exact,
deterministic or atomic-free — for these families all of it, with the two remarks below — is also equal in bits between the
two runs.  A kernel that relies on a zeroed workspace word, or leaves an output element unwritten at an odd shape, fails the
second run.  tests/test_fuzz_gpu.py::test_dirty_allocator_positive_control shows that the helper does what the second runs
rely on.

  * fastrcnn_loss, mask_loss and rpn_loss: the header states the fixed summation order for the keypoint loss only; the
    others' kernels (csrc/head_loss.hip, csrc/targets.hip) hold no floating-point atomic either and sum per-row partials
    from the workspace in index order, so the same is asked of them.
  * rpn_head_sparse: the header promises a deterministic BACKWARD.  Its forward is the library's convolutions, which need
    not add in the same order from call to call; the backward is therefore asked to reproduce itself on one saved forward in
    every run, and between the clean and the dirty run wherever the two forwards agree in bits (they do with
    torch.backends.cudnn.deterministic, which the test sets; otherwise the test says so and compares by tolerance only).

Bounds: tests/fuzz_ext_runs.py names each.  Measured on an MI355X over each family's seeds (FIGURE lines, run with -s):
    family / kernel      worst value   worst gradient / array   held to (value, gradient / array)
    roi_head_targets     -             3.62e-06                 -, 2.90e-05     (ATen fp32 encode on the same slots: 3.62e-06)
    fastrcnn_loss        5.35e-06      2.71e-06                 4.28e-05, 4.62e-05   (ATen fp32: 5.35e-06, 5.78e-06)
    mask_loss            9.03e-08      1.71e-07                 8.16e-07, 1.45e-06   (ATen fp32: 6.86e-08, 1.82e-07)
    keypoint_loss        8.80e-08      1.11e-06                 1e-05, 1e-05
    rpn_loss             1.13e-07      6.18e-07                 7.91e-07, 4.13e-06   (ATen fp32: 9.22e-08, 5.16e-07)
    rpn_head_sparse      largest relative Frobenius spread 2.93e-07, held to GRAD_TOL = 4e-05; the two forwards agreed in bits on
                         every seed
    group_norm           of their bounds: mean 0.04, rstd 0.11, output 0.63; backward error over 8 x ATen's (or the half-type
                         floor): grad_x 0.32, grad_gamma 0.17, grad_beta 0.09
    bias_act             bias gradient 1.62e-05 (256 channels x 4097 rows of bf16), column_sum 6.68e-06, held to 1e-5 x
                         max(1, largest column sum of magnitudes): 3.3e-02 and 8.0e-03 on those two cases
    rpn_decode, targets, sampler, labels, mask_chain, bbox_aug_merge: exact
  The bounds of the first rows: BOUNDS of tests/test_targets_edges_gpu.py where the drawn cases stay inside them; a drawn case
  may be conditioned worse than the hand-picked ones (one sampled slot whose target is small; one row whose two logits nearly
  cancel), so each is the larger of BOUNDS and 8 x the worst error, over the family's seeds, of the plain fp32 ATen composition
  of the same operation against the same fp64 reference (tests/fuzz_ext_runs.py::bounds_of) — computed from ATen, never from
  the kernel.  The kernels' worst figures sit on the same two cases as ATen's.
  The whole file takes under ten seconds on an MI355X; the slowest case 2.5 s (the first sparse backward: library warm-up)."""
import pytest
import torch

import fuzz_cases
import fuzz_ext_runs as X
from dirty_memory import _clean_then_dirty, dirty_allocator
from graph_replay import bits_equal, first_difference

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = fuzz_cases.SEEDS


def _sweep(family, seed):
    c = fuzz_cases.FAMILIES[family](seed)
    assert c is not None
    r = X.refs(family, seed)
    _clean_then_dirty(lambda: X.RUN[family](c, r, DEV))


@pytest.mark.parametrize("seed", range(SEEDS["targets_chain"]))
def test_fuzz_targets_chain(seed):
    """match_boxes -> match_labels -> sample_labels(with_list) -> roi_head_targets, each fed the previous one's device output:
    the matcher's per-gt maxima and the sampler's counters, candidate lists and key thresholds live in torch.empty workspaces"""
    _sweep("targets_chain", seed)


@pytest.mark.parametrize("seed", range(SEEDS["head_losses"]))
def test_fuzz_head_losses(seed):
    """fastrcnn_loss, mask_loss and keypoint_loss forward and backward through the autograd nodes: per-row partial sums and
    the sample count go through the workspace, the stored gradients through torch.empty_like"""
    _sweep("head_losses", seed)


@pytest.mark.parametrize("seed", range(SEEDS["rpn_loss_decode"]))
def test_fuzz_rpn_loss_decode(seed):
    """rpn_loss forward and backward over 1..8 levels, and rpn_decode per level at non-zero col / off behind NaN guard columns"""
    _sweep("rpn_loss_decode", seed)


@pytest.mark.parametrize("seed", range(SEEDS["rpn_head_sparse"]))
def test_fuzz_rpn_head_sparse(seed, monkeypatch):
    """the sparse RPN-head backward: its row lists are built on the device in rounds of 256 candidates inside a torch.empty
    workspace; on the overflow seed grad_w_conv is all NaN, the counter rises and everything else stays finite"""
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", False)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    c, r = fuzz_cases.rpn_head_sparse(seed), X.refs("rpn_head_sparse", seed)
    clean = {k: v.cpu() for k, v in X.RUN["rpn_head_sparse"](c, r, DEV).items()}
    dirty_allocator()
    dirty = X.RUN["rpn_head_sparse"](c, r, DEV)
    assert sorted(clean) == sorted(dirty)
    if not all(bits_equal(clean[k], dirty[k]) for k in clean if k.startswith("forward_")):
        print("the two forwards differ in bits: the backward is compared with the reference only")
        return
    for k in sorted(clean):
        assert bits_equal(clean[k], dirty[k]), "%s differs between clean and dirty memory: %s" % (k, first_difference(clean[k], dirty[k]))


@pytest.mark.parametrize("seed", range(SEEDS["mask_chain"]))
def test_fuzz_mask_chain(seed):
    """paste_masks -> paste_masks_rle -> rle_strings -> rle_string_decode -> mask_pack_rle / mask_pack -> mask_pair_counts ->
    eval_iou -> eval_match on one set of detections: three count / host read / write pairs whose workspace must survive
    between the two calls, and the four launches of mask_pack_rle"""
    _sweep("mask_chain", seed)


@pytest.mark.parametrize("seed", range(SEEDS["bbox_aug_merge"]))
def test_fuzz_bbox_aug_merge(seed):
    """the merge of test-time augmentation: count, one host read, write, through one workspace"""
    _sweep("bbox_aug_merge", seed)


@pytest.mark.parametrize("seed", range(SEEDS["group_norm"]))
def test_fuzz_group_norm(seed):
    """channels-last GroupNorm (+ residual) (+ ReLU) forward and backward: per-workgroup partial statistics and the gamma /
    beta partial sums of the split regime go through the workspace"""
    _sweep("group_norm", seed)


@pytest.mark.parametrize("seed", range(SEEDS["bias_act"]))
def test_fuzz_bias_act(seed):
    """the fused bias (+ ReLU) pass, its backward with the bias gradient, and column_sum: per-workgroup partial column sums in
    the workspace, added in index order by a second launch"""
    _sweep("bias_act", seed)
