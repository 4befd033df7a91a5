"""COCO result files on the MI355X (`-m gpu`): the kernels of csrc/rle_string.hip (`_C.rle_strings`) against the numpy
statement of the same definition (`_rle_cpu.rle_strings`, itself pinned to the literal coder by
tests/test_coco_results_cpu.py), bytes and offsets exactly; then `COCOResultsWriter` on device tensors against its CPU path.

The string coding is integer arithmetic: everything here is exact.  The end-to-end case compares masks pasted by
csrc/masker.hip with masks pasted by ATen; the two restate one fp32 resize and may land on different sides of the threshold
where the interpolated value lies within 1e-5 of it (tests/test_masker_gpu.py).  The case's inputs are checked, on the
CPU, to have no such pixel."""
import json

import numpy as np
import pytest
import torch

import rle_string_refs as R
from maskrcnn_benchmark import _lib, _rle_cpu
from maskrcnn_benchmark.data.datasets.evaluation import coco_results as CR
from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import paste_masks_torch
from maskrcnn_benchmark.structures.bounding_box import BoxList

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 1024          # kChunk of csrc/rle_string.hip: runs of the flat array per workgroup
GUARD = 64
EINVAL, EWORKSPACE = -1, -2


def _C():
    from maskrcnn_benchmark import _C as c
    return c


def _flat(masks):
    counts = np.concatenate([np.asarray(m, np.int32) for m in masks] + [np.zeros(0, np.int32)])
    return counts, np.concatenate([[0], np.cumsum([len(m) for m in masks])]).astype(np.int64)


def _runs(rng, n):
    """n runs as masks have them: mostly short, some long, so that deltas take 1 to 4 bytes with both signs"""
    return np.where(rng.rand(n) < 0.8, rng.randint(0, 40, n), rng.randint(0, 70000, n)).astype(np.int32).tolist()


def _raw(counts, run_offset, shift):
    """the two entry points themselves, the output at `shift` bytes past a 16-byte boundary inside a buffer of 0xAB
    -> (bytes, byte_offset, the buffer's bytes in front of and behind the output), on the host"""
    lib, ptr = _lib.lib, _lib.ptr
    c, ro = torch.from_numpy(counts).to(DEV), torch.from_numpy(run_offset).to(DEV)
    total, N = c.numel(), ro.numel() - 1
    nbytes = int(lib.detops_rle_string_workspace_bytes(total))
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=DEV)
    byte_offset = torch.zeros((N + 1,), dtype=torch.int64, device=DEV)
    assert lib.detops_rle_string_count(ptr(c), ptr(ro), total, N, ptr(byte_offset), ptr(ws), nbytes, None) == 0
    B = int(byte_offset[-1].item())
    buf = torch.full((B + 2 * GUARD + 32,), 0xAB, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 16 + GUARD - GUARD % 16 + shift
    out = buf[start:start + B]
    assert (out.data_ptr() % 16 == shift % 16) or B == 0
    assert lib.detops_rle_string_write(ptr(c), ptr(ro), total, N, ptr(byte_offset), out.data_ptr(), ptr(ws), nbytes, None) == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return host[start:start + B], byte_offset.cpu().numpy(), np.concatenate([host[:start], host[start + B:]])


def _check(masks, shifts=(0,)):
    counts, run_offset = _flat(masks)
    want, want_off = _rle_cpu.rle_strings(counts, run_offset)
    data, off = _C().rle_strings(torch.from_numpy(counts).to(DEV), torch.from_numpy(run_offset).to(DEV))
    assert data.is_cuda and off.is_cuda and data.dtype == torch.uint8 and off.dtype == torch.int64
    assert np.array_equal(off.cpu().numpy(), want_off)
    assert np.array_equal(data.cpu().numpy(), want)
    assert _C().rle_string_list(data, off) == _rle_cpu.to_str_list(want, want_off)
    for shift in shifts:
        got, got_off, guard = _raw(counts, run_offset, shift)
        assert np.array_equal(got_off, want_off) and np.array_equal(got, want), shift
        assert (guard == 0xAB).all(), "shift %d: bytes outside the output were written" % shift
    return want, want_off


def test_no_masks_and_no_runs():
    c = _C()
    data, off = c.rle_strings(torch.empty(0, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV))
    assert data.numel() == 0 and data.is_cuda and off.tolist() == [0] and c.rle_string_list(data, off) == []
    data, off = c.rle_strings(torch.empty(0, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV))
    assert data.numel() == 0 and off.tolist() == [0, 0, 0, 0] and c.rle_string_list(data, off) == ["", "", ""]


def test_the_eight_vectors():
    want, off = _check([c for c, _ in R.VECTORS])
    assert _rle_cpu.to_str_list(want, off) == [t for _, t in R.VECTORS]
    for counts, text in R.VECTORS:
        data, o = _C().rle_strings(torch.tensor(counts, dtype=torch.int32, device=DEV), torch.tensor([0, len(counts)], device=DEV))
        assert _C().rle_string_list(data, o) == [text]


def test_masks_of_one_to_four_runs():
    rng = np.random.RandomState(1)
    for n in (1, 2, 3, 4):
        _check([_runs(rng, n)])
    _check([_runs(rng, n) for n in (1, 2, 3, 4, 4, 3, 2, 1)] + [[], [7], []], shifts=(0, 1))


def test_chunk_boundaries_inside_masks_and_mask_boundaries_inside_chunks():
    rng = np.random.RandomState(2)
    _check([[5], _runs(rng, 257), [6], _runs(rng, CHUNK + 1), [7]], shifts=(0, 5))
    # a chunk boundary at run index 0, 1, 2, 3 and 4 of a mask: masks of one run in front of it
    for lead in (CHUNK, CHUNK - 1, CHUNK - 2, CHUNK - 3, CHUNK - 4):
        _check([[3]] * lead + [_runs(rng, 9)] + [[4]] * 3)
    _check([_runs(rng, CHUNK)] + [_runs(rng, CHUNK)])          # masks that are exactly a chunk


@pytest.mark.parametrize("total", [1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_total_runs_around_one_chunk(total):
    """one chunk, not quite full and full, and one chunk plus one run; masks without runs in front, inside and behind"""
    rng = np.random.RandomState(total)
    runs = _runs(rng, total)
    _check([runs])
    cut = total // 2
    _check([[], runs[:cut], [], [], runs[cut:], []], shifts=(0, 7))


def test_more_chunks_than_the_offsets_scan_has_threads():
    """257 chunks: the scan over the chunks' bytes carries across its tile of 256; masks without runs at the start, at a chunk
    boundary (the tile's boundary among them) and at the end"""
    rng = np.random.RandomState(8)
    masks = [[], [], _runs(rng, 100 * CHUNK), [], _runs(rng, 156 * CHUNK), [], [], _runs(rng, CHUNK - 5), [1, 2, 3, 4, 5], [], []]
    assert sum(len(m) for m in masks) == 257 * CHUNK
    _check(masks)


def test_an_interior_mask_of_many_runs_between_tiny_ones():
    rng = np.random.RandomState(3)
    _check([[1], [2, 3], _runs(rng, 5 * CHUNK + 77), [4], [], [5, 6, 7]], shifts=(0, 9))


def test_seven_byte_values_and_every_shorter_length():
    big = 2 ** 31 - 1
    masks = [[big, 0, 0, 0, big, 0, 0, big], [0, big, 0, 0], [big] * 6, R.EDGE_VALUES, R.EDGE_VALUES[::-1]] + R.seeded_masks(300, seed=4)
    want, off = _check(masks, shifts=(0, 3))
    lengths = _rle_cpu.code_lengths(_rle_cpu.deltas(*_flat(masks)))
    assert set(lengths.tolist()) == set(range(1, 8))
    assert _rle_cpu.to_str_list(want, off)[0] == R.rle_to_string(masks[0])


def test_unaligned_head_and_tail_of_the_wide_stores():
    """an output whose total is not a multiple of 16, at every alignment of its first byte; masks at odd byte offsets"""
    rng = np.random.RandomState(5)
    masks = [[1, 2, 3], _runs(rng, 700), [9], _runs(rng, 2 * CHUNK + 3), [4, 4, 4]]
    want, off = _check(masks, shifts=tuple(range(16)))
    assert want.size % 16 != 0 and any(o % 2 for o in off.tolist())
    _check([[1]], shifts=(0, 15))                              # one byte: no full line at all
    _check([[100] * 15], shifts=(1,))                          # the head reaches the boundary exactly
    _check([[100] * 17], shifts=(15,))


def test_two_calls_give_identical_bytes():
    rng = np.random.RandomState(6)
    counts, run_offset = _flat([_runs(rng, n) for n in (3000, 1, 40, 2049, 2)])
    c, ro = torch.from_numpy(counts).to(DEV), torch.from_numpy(run_offset).to(DEV)
    a, b = _C().rle_strings(c, ro), _C().rle_strings(c, ro)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_error_codes():
    lib, ptr = _lib.lib, _lib.ptr
    c = torch.ones(8, dtype=torch.int32, device=DEV)
    ro = torch.tensor([0, 8], device=DEV)
    off = torch.zeros(2, dtype=torch.int64, device=DEV)
    out = torch.zeros(64, dtype=torch.uint8, device=DEV)
    nbytes = int(lib.detops_rle_string_workspace_bytes(8))
    assert nbytes > 0 and lib.detops_rle_string_workspace_bytes(0) == 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    count, write = lib.detops_rle_string_count, lib.detops_rle_string_write
    assert count(ptr(c), ptr(ro), -1, 1, ptr(off), ptr(ws), nbytes, None) == EINVAL
    assert count(ptr(c), ptr(ro), 8, -1, ptr(off), ptr(ws), nbytes, None) == EINVAL
    assert count(None, ptr(ro), 8, 1, ptr(off), ptr(ws), nbytes, None) == EINVAL
    assert count(ptr(c), None, 8, 1, ptr(off), ptr(ws), nbytes, None) == EINVAL
    assert count(ptr(c), ptr(ro), 8, 1, None, ptr(ws), nbytes, None) == EINVAL
    assert count(ptr(c), ptr(ro), 8, 1, ptr(off), None, nbytes, None) == EINVAL
    assert count(ptr(c), ptr(ro), 8, 1, ptr(off), ptr(ws), nbytes - 1, None) == EWORKSPACE
    assert write(ptr(c), ptr(ro), 8, 1, ptr(off), None, ptr(ws), nbytes, None) == EINVAL
    assert write(ptr(c), ptr(ro), -1, 1, ptr(off), ptr(out), ptr(ws), nbytes, None) == EINVAL
    assert write(ptr(c), ptr(ro), 8, 1, ptr(off), ptr(out), ptr(ws), nbytes - 1, None) == EWORKSPACE
    assert count(None, None, 0, 5, None, None, 0, None) == 0 and count(None, None, 8, 0, None, None, 0, None) == 0
    assert write(None, None, 0, 5, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert off.tolist() == [0, 0] and int(out.sum()) == 0       # nothing was launched
    with pytest.raises(ValueError):
        _C().rle_strings(c.long(), ro)
    with pytest.raises(ValueError):
        _C().rle_strings(c, ro.cpu())


# ------------------------------------------------------------------------------------------------ end to end
H, W = 97, 131
IMAGES = [{"id": 42, "width": W, "height": H}]
# xyxy in the prediction's frame, 262 x 194 (twice the image: the resize to the original size is exact); in the image:
BOXES = [[-20, 20, 60, 90], [30, -16, 120, 50], [200, 60, 290, 150], [100, 150, 180, 230],      # left, top, right, bottom border
         [-10, -10, 40, 40], [220, 150, 300, 220], [-30, -30, 300, 230],                        # two corners, all four borders
         [400, 60, 500, 150],                                                                   # misses the image
         [60, 40, 200, 160], [10, 10, 16, 14], [128, 96, 131, 99], [0, 0, 261, 193]]


class _Dataset(object):
    id_to_img_map = {0: 42}
    contiguous_category_id_to_json_id = {1: 5, 2: 17, 3: 80}

    def get_img_info(self, index):
        return IMAGES[index]


def _prediction(mask):
    g = torch.Generator().manual_seed(21)
    p = BoxList(torch.tensor(BOXES, dtype=torch.float32), (2 * W, 2 * H), mode="xyxy")
    p.add_field("scores", torch.rand(len(BOXES), generator=g))
    p.add_field("labels", torch.randint(1, 4, (len(BOXES),), generator=g))
    p.add_field("mask", mask)
    return p


def _entries(prediction, device):
    writer = CR.COCOResultsWriter(_Dataset(), ("bbox", "segm"))
    writer.update([prediction.to(device)], [0])
    return json.loads(json.dumps(writer.results))               # what the files hold


def test_writer_on_device_probabilities_equals_the_cpu_path():
    g = torch.Generator().manual_seed(2026)      # a seed for which the assertion two lines down holds
    prob = torch.rand(len(BOXES), 1, 28, 28, generator=g)
    boxes = torch.tensor(BOXES, dtype=torch.float32) * 0.5
    lo, hi = (paste_masks_torch(prob, boxes, H, W, t, 1) for t in (0.5 - 1e-5, 0.5 + 1e-5))
    assert torch.equal(lo, hi), "the case has pixels within 1e-5 of the threshold: choose another seed"
    p = _prediction(prob)
    cpu, dev = _entries(p, "cpu"), _entries(p, DEV)
    assert dev == cpu and len(dev["segm"]) == len(dev["bbox"]) == 12
    planes = paste_masks_torch(prob, boxes, H, W, 0.5, 1)
    for k, e in enumerate(dev["segm"]):
        assert e["segmentation"]["size"] == [H, W] and e["image_id"] == 42
        runs = R.rle_from_string(e["segmentation"]["counts"])
        assert sum(runs) == H * W and sum(runs[1::2]) == int(planes[k].sum())
    assert dev["segm"][7]["segmentation"]["counts"] == R.rle_to_string([H * W])      # the box that misses the image
    assert all(int(planes[k].sum()) > 0 for k in range(12) if k != 7)


def test_writer_on_device_dense_planes_equals_the_cpu_path():
    g = torch.Generator().manual_seed(8)
    planes = torch.rand(len(BOXES), 1, H, W, generator=g) > 0.7
    planes[3] = False
    planes[4] = True
    p = _prediction(planes)
    cpu, dev = _entries(p, "cpu"), _entries(p, DEV)
    assert dev == cpu
    assert dev["segm"][3]["segmentation"]["counts"] == R.rle_to_string([H * W])
    assert dev["segm"][4]["segmentation"]["counts"] == R.rle_to_string([0, H * W])
