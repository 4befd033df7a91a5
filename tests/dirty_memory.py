"""Uninitialised device memory for the seeded sweeps (tests/test_fuzz_gpu.py, tests/test_fuzz_ext_gpu.py).

A plain module: no tests, no fixtures.  `_C` takes every output and workspace from `torch.empty`, and a test process mostly
hands out fresh (zero) pages.  `dirty_allocator()` leaves 0xFF bytes — NaN in every float type, -1 in every integer type — in
the free blocks that the next allocations are cut from; `_clean_then_dirty(run)` runs a case once on the allocator as it is and
once on such memory.  tests/test_fuzz_gpu.py::test_dirty_allocator_positive_control shows that the helper does what the
second runs rely on."""
import numpy as np
import torch

from graph_replay import bits_equal, first_difference

DEV = "cuda"


def _claim_free_blocks():
    """-> uint8 tensors that occupy every free block of the current device's and stream's allocator pools (read from
    `torch.cuda.memory_snapshot()`): each block is asked for by its own size, which best fit answers with a block of exactly
    that size; the small pool serves requests up to 1 MB, so a larger remainder of one of its 2 MB segments goes in two
    rounds.  Blocks of other streams' pools stay: no allocation of the current stream is cut from them."""
    device, stream = torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream
    held, before = [], None
    for _ in range(8):
        sizes = []
        for seg in torch.cuda.memory_snapshot():
            if seg["device"] != device or seg.get("stream", stream) != stream:
                continue
            small = seg["segment_type"] == "small"
            for b in seg["blocks"]:
                if b["state"] == "inactive" and (small or b["size"] > (1 << 20)):
                    sizes.append(min(b["size"], 1 << 20) if small else b["size"])
        sizes.sort(reverse=True)
        if not sizes or sizes == before:
            break
        before = sizes
        held += [torch.empty((n,), dtype=torch.uint8, device=DEV) for n in sizes]
    return held


def dirty_allocator():
    """Leave 0xFF bytes in the caching allocator's free blocks: after a sync and `empty_cache()` (nothing cached: the next
    blocks come from the driver), one 64 MB and two 1 MB uint8 tensors — a split-able block in the large pool (requests
    above 1 MB) and one in the small pool — are filled, synchronised and freed.  The allocations that follow are cut from
    these blocks.  0xFF reads as NaN in every float type and as -1 in every integer type (graph_replay.poison_); a quiet-NaN
    pattern would read as a large positive index.
    `empty_cache()` cannot release a segment that a live tensor sits in (tensors that earlier tests of the session or the
    library keep: status words, cached plans), and the best-fit allocator serves a request from the smallest free block
    that fits — such a segment's stale remainder before the fresh blocks.  So every free block left in the current stream's
    pools is claimed first, by a request of its own size, and filled like the others."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    blocks = _claim_free_blocks()
    blocks += [torch.empty((64 << 20,), dtype=torch.uint8, device=DEV),
               torch.empty((1 << 20,), dtype=torch.uint8, device=DEV), torch.empty((1 << 20,), dtype=torch.uint8, device=DEV)]
    for b in blocks:
        b.fill_(0xFF)
    torch.cuda.synchronize()
    del b, blocks


def _clean_then_dirty(run):
    """run() -> dict name -> tensor of what must be reproducible; once as is, once on dirtied free blocks; both runs assert
    against the reference themselves, and the reproducible outputs of the second equal those of the first in bits.  The
    first run's outputs move to the host before the allocator is dirtied: a live device tensor would keep its segment
    cached, and the best-fit allocator would serve the second run from that segment's stale remainder first"""
    clean = {name: t.cpu() for name, t in run().items()}
    dirty_allocator()
    dirty = run()
    assert sorted(clean) == sorted(dirty)
    for name in sorted(clean):
        assert bits_equal(clean[name], dirty[name]), "%s differs between clean and dirty memory: %s" % (
            name, first_difference(clean[name], dirty[name]))


def _within(got, ref, tol, what):
    err = float(np.abs(got - ref).max()) if got.size else 0.0      # NaN (an element left unwritten) fails the comparison
    assert err <= tol, (what, err, tol)
