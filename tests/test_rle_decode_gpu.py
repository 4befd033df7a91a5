"""Device checks of reading compressed RLE strings (csrc/rle_decode.hip) and of packing runs into bit rows
(detops_mask_pack_rle of csrc/evaluate.hip): everything is compared EXACTLY with the numpy statements of the same
definitions (_rle_cpu.py, _eval_cpu.py), which tests/test_rle_decode_cpu.py pins to the literal decoder of
rle_string_refs.py."""
import numpy as np
import pytest
import torch

import eval_cases as C
import rle_decode_cases as K
import rle_string_refs as R
from maskrcnn_benchmark import _eval_cpu, _rle_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 2048          # bytes of a workgroup of csrc/rle_decode.hip (kChunk)
GUARD = 3


def guarded(n, dtype, fill, guard=GUARD):
    t = torch.full((n + 2 * guard,), fill, dtype=dtype, device=DEV)
    return t, t[guard:guard + n]


def untouched(t, fill, guard=GUARD):
    return bool((t[:guard] == fill).all()) and bool((t[-guard:] == fill).all())


def decode_with_guards(strings, hw=None):
    """the two entry points called as the wrapper calls them, on outputs with guard elements on both sides"""
    from maskrcnn_benchmark._lib import check, lib, ptr

    data, bo = K.tensors(strings, DEV)
    B, N = data.numel(), bo.numel() - 1
    nbytes = int(lib.detops_rle_decode_workspace_bytes(B, N))
    ws_all, ws = guarded(nbytes, torch.uint8, 0xAB, 8)        # (the workspace holds 64-bit words: keep it aligned)
    ro_all, ro = guarded(N + 1, torch.int64, -7)
    check(lib.detops_rle_decode_count(ptr(data), ptr(bo), B, N, ptr(ro), ptr(ws), nbytes, None), "count")
    torch.cuda.synchronize()
    total = int(ro[-1]) if B and N else 0
    counts_all, counts = guarded(total, torch.int32, -7)
    status_all, status = guarded(N, torch.int32, -7)
    hw_d = None if hw is None else torch.tensor(hw, dtype=torch.int32).reshape(-1, 2).to(DEV)
    check(lib.detops_rle_decode_write(ptr(data), ptr(bo), B, N, ptr(ro), total, ptr(hw_d), ptr(counts), ptr(status), ptr(ws),
                                      nbytes, None), "write")
    torch.cuda.synchronize()
    assert untouched(ws_all, 0xAB, 8) and untouched(ro_all, -7) and untouched(counts_all, -7) and untouched(status_all, -7)
    return counts.cpu().numpy(), ro.cpu().numpy(), status.cpu().numpy()


def numpy_decode(strings, hw=None):
    return _rle_cpu.rle_decode(*_rle_cpu.from_str_list(strings), hw)


def same_decode(strings, hw=None):
    """guarded entry points == the wrapper == numpy, in counts, run_offset and status; -> numpy's"""
    from maskrcnn_benchmark import _C

    want = numpy_decode(strings, hw)
    got = decode_with_guards(strings, hw)
    wrapped = _C.rle_string_decode_status(*K.tensors(strings, DEV), hw)
    for w, g, t, name in zip(want, got, wrapped, ("counts", "run_offset", "status")):
        np.testing.assert_array_equal(g, w, err_msg=name)
        assert t.is_cuda and t.dtype == torch.from_numpy(w).dtype
        np.testing.assert_array_equal(t.cpu().numpy(), w, err_msg=name + " (wrapper)")
    return want


# ------------------------------------------------------------------ decode
def test_seeded_strings_concatenated():
    """2,000 strings back to back: mask and value boundaries at every position of a chunk, 1 to 7 bytes per value"""
    masks, strings = K.seeded_strings()
    counts, ro, status = same_decode(strings)
    assert not status.any() and ro[-1] == sum(len(m) for m in masks)
    assert counts.tolist() == [v for m in masks for v in m]
    assert sum(len(s) for s in strings) > 8 * CHUNK


@pytest.mark.parametrize("shift", range(1, 7))
def test_a_seven_byte_value_split_across_two_chunks(shift):
    """`shift` bytes of the value lie in the first chunk"""
    runs = [1] * (CHUNK - shift) + [2 ** 31 - 1, 5]
    s = R.rle_to_string(runs)
    assert R.code_length(2 ** 31 - 2) == 7 and len(s) == CHUNK + 7 - shift + 1
    counts, _, status = same_decode(["0", s, "53"])
    assert counts.tolist() == [0] + runs + [5, 3] and not status.any()


def test_one_long_mask_next_to_short_ones():
    masks, strings = K.long_and_short()
    counts, ro, status = same_decode(strings, [(0, 9), (7, 1), (1, sum(masks[2])), (2, 3), (0, 0)])
    assert ro.tolist() == [0, 0, 1, 50001, 50004, 50004] and not status.any()
    assert counts[1:50001].tolist() == masks[2]


def test_one_mask_no_mask_and_only_empty_strings():
    from maskrcnn_benchmark import _C

    counts, ro, status = same_decode([R.VECTORS[4][1]], [(5, 10)])
    assert counts.tolist() == R.VECTORS[4][0] and status.tolist() == [0]
    for strings, hw in (([], None), (["", "", ""], None), (["", ""], [(0, 3), (1, 1)])):
        want = numpy_decode(strings, hw)
        got = decode_with_guards(strings, hw)            # the entry points launch nothing and write nothing
        assert got[0].size == 0 and (got[1] == -7).all() and (got[2] == -7).all()
        wrapped = _C.rle_string_decode_status(*K.tensors(strings, DEV), hw)
        for w, t in zip(want, wrapped):
            np.testing.assert_array_equal(t.cpu().numpy(), w)


def test_malformed_strings_are_data():
    """every malformed case: the status numpy gives, no fault, nothing outside the arrays; the well-formed neighbours of a
    malformed string decode as if alone"""
    from maskrcnn_benchmark import _C

    strings = [s for s, _, _, _ in K.MALFORMED]
    hw = [h for _, h, _, _ in K.MALFORMED]
    _, _, status = same_decode(strings, hw)
    assert status.tolist() == [whole for _, _, _, whole in K.MALFORMED]
    for n in range(len(strings)):
        if strings[n]:         # (a call of empty strings only launches nothing: test_one_mask_no_mask_and_only_empty_strings)
            same_decode(strings[n:n + 1], hw[n:n + 1])
    mixed = ["053", strings[0], "?`0a0A", strings[3], "P]aP1"]
    counts, ro, status = same_decode(mixed)
    assert status.tolist() == [0, 11, 0, 4, 0]
    assert counts[ro[0]:ro[1]].tolist() == [0, 5, 3] and counts[ro[2]:ro[3]].tolist() == [15, 16, 17, 1]
    with pytest.raises(ValueError, match=r"mask 1 .*status 11.*DETOPS_RLE_BAD_BYTE"):
        _C.rle_string_decode(*K.tensors(mixed, DEV))
    random_bytes = bytes(np.random.RandomState(1).randint(0, 256, 5000).astype(np.uint8).tolist()).decode("latin-1")
    same_decode([random_bytes[:1234], random_bytes[1234:1234], random_bytes[1234:]], [(3, 4), (0, 0), (5, 6)])


def test_decode_list_crosses_in_one_copy():
    from maskrcnn_benchmark import _C

    masks, strings = K.seeded_strings()
    counts, ro = _C.rle_string_decode_list(strings[:50], None, DEV)
    assert counts.is_cuda and counts.tolist() == [v for m in masks[:50] for v in m]
    with pytest.raises(ValueError, match="mask 2 .*DETOPS_RLE_BAD_SUM"):
        _C.rle_string_decode_list(["053", "44", "053"], [(2, 4), (2, 4), (3, 3)], DEV)


# ------------------------------------------------------------------ pack
def same_pack(got, want):
    for g, w, name in zip(got, want, ("words", "word_offset", "hw", "area", "extent")):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w.cpu()), name


def numpy_pack(planes):
    w, off, hw, area, ext = _eval_cpu.mask_pack([p[None] for p in planes])
    return tuple(torch.from_numpy(a) for a in (w.view(np.int64), off, hw, area, ext))


def test_pack_from_runs_as_one_call_of_mixed_sizes():
    from maskrcnn_benchmark import _C

    planes, runs = K.pack_cases(extra_h=(_C.MASK_PACK_RLE_MAX_H,))
    assert max(p.shape[0] for p in planes) == _C.MASK_PACK_RLE_MAX_H == 4096
    hw = [p.shape for p in planes]
    want = numpy_pack(planes)
    same_pack(_C.mask_pack_rle(*K.run_tensors(runs), hw), want)            # CPU tensors: numpy
    got = _C.mask_pack_rle(*K.run_tensors(runs, DEV), hw)
    assert all(t.is_cuda for t in got)
    same_pack(got, want)
    same_pack(_C.mask_pack_rle(*K.run_tensors(runs, DEV), hw), want)       # a second run: identical


def test_pack_above_the_cap_takes_the_numpy_path():
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark._lib import lib

    planes, runs = K.pack_cases(extra_h=(_C.MASK_PACK_RLE_MAX_H + 1,))
    got = _C.mask_pack_rle(*K.run_tensors(runs, DEV), [p.shape for p in planes])
    assert all(t.is_cuda for t in got)
    same_pack(got, numpy_pack(planes))
    assert lib.detops_mask_pack_rle(None, None, 0, None, 1, _C.MASK_PACK_RLE_MAX_H + 1, 3, None, None, None, None, None, 0,
                                    None) == -3     # DETOPS_EUNSUPPORTED, nothing launched


def test_pack_of_pasted_runs_equals_pack_of_pasted_planes():
    """5 detections on a 40 x 72 image: boxes clipped at every border, one box outside the image"""
    from maskrcnn_benchmark import _C

    H, W = 40, 72
    boxes = torch.tensor([[-9.5, 4.0, 20.0, 30.0], [50.0, -6.0, 90.5, 20.0], [10.0, 25.0, 60.0, 55.0], [-5.0, -5.0, 80.0, 50.0],
                          [100.0, 100.0, 130.0, 140.0]], device=DEV)
    probs = torch.sigmoid(3 * torch.randn(5, 1, 28, 28, generator=torch.Generator().manual_seed(4))).to(DEV)
    counts, run_offset = _C.paste_masks_rle(probs, boxes, [(H, W)], counts=[5])
    _, views = _C.paste_masks(probs, boxes, [(H, W)], counts=[5])
    want = _C.mask_pack([views[0][:, 0]])
    assert 0 < int(want[3][:4].min()) and int(want[3][4]) == 0
    same_pack(_C.mask_pack_rle(counts, run_offset, [(H, W)] * 5), want)


# ------------------------------------------------------------------ evaluator
def test_evaluator_on_device_rle_masks_equals_dense_planes():
    from maskrcnn_benchmark.data.datasets.evaluation import COCOStyleEvaluator
    from maskrcnn_benchmark.data.datasets.evaluation.coco_results import plane_runs
    from maskrcnn_benchmark.structures.rle_masks import RLEMasks

    images = C.make_images()
    preds, tgts = C.to_boxlists(images, DEV)
    want = COCOStyleEvaluator(("bbox", "segm"), C.NUM_CLASSES)
    want.update(preds, tgts)
    want.summarize()
    rle_preds = []
    for p in preds:
        q = p.copy_with_fields(["scores", "labels"])
        q.add_field("mask", RLEMasks(*plane_runs(p.get_field("mask")[:, 0]), p.size))
        rle_preds.append(q)
    assert rle_preds[0].get_field("mask").counts.is_cuda
    tgts[3].add_field("masks", RLEMasks(*plane_runs(tgts[3].get_field("masks").instances.masks), tgts[3].size))
    ev = COCOStyleEvaluator(("bbox", "segm"), C.NUM_CLASSES)
    ev.update(rle_preds[:5], tgts[:5])
    ev.update(rle_preds[5:], tgts[5:])
    ev.summarize()
    for iou_type in ("bbox", "segm"):
        ra, rb = C.records_by_key(ev, iou_type), C.records_by_key(want, iou_type)
        assert sorted(ra) == sorted(rb)
        for key in rb:
            for field in ("scores", "dt_match", "dt_ignore", "gt_ignore"):
                np.testing.assert_array_equal(ra[key][field], rb[key][field], err_msg="%s %s %s" % (iou_type, key, field))
        np.testing.assert_array_equal(ev.stats[iou_type], want.stats[iou_type])
    assert 0 < ev.stats["segm"][0] < 1
