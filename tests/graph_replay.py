"""Replay harness for the sync-free operators: one capture into a HIP graph, replays with changing values, every replay
held against an eager call (and a reference) of the same values.  Used by tests/test_graph_replay_gpu.py.

A plain module: no tests, no fixtures.  A capture freezes launch arguments, workspace addresses and every decision the
host took while capturing; `check_replay` looks for each way that goes wrong:
  * the values change between replays (other data-dependent routes than at capture);
  * every captured output is overwritten with a poison pattern before each replay (an output the replay does not write);
  * between two replays the operator runs once eagerly at another shape (`between`: status words, cached workspaces and
    plans shared by eager calls and the graph);
  * the first value set comes back at the end, and is then replayed once more without reloading the inputs (state a
    replay leaves behind for the next one);
  * the eager call that the replay is compared with runs AFTER the replay, on fresh tensors.
Comparison is of bits (integer views: NaN equals NaN, -0.0 differs from 0.0) unless the caller passes a comparison of its
own."""
import numpy as np
import torch

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# ------------------------------------------------------------------------------------------ pure helpers (CPU-testable)
def as_tensor(a):
    """numpy array / tensor / None -> tensor / None (no copy where avoidable)"""
    if a is None or torch.is_tensor(a):
        return a
    return torch.from_numpy(np.ascontiguousarray(a))


def bit_view(t):
    """the tensor's bits as integers of the same width, in logical (index) order: equal views <=> equal bits"""
    t = t.detach()
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    if t.is_complex():
        raise TypeError("bit_view: complex tensors are not supported")
    if not t.is_floating_point():
        return t.contiguous()
    return t.contiguous().view(_INT_VIEW[t.element_size()])


def bits_equal(a, b):
    a, b = as_tensor(a), as_tensor(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bit_view(a).cpu(), bit_view(b).cpu()))


def first_difference(a, b):
    """a short description of where two tensors differ in bits (for assertion messages)"""
    a, b = as_tensor(a), as_tensor(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return "%s %s vs %s %s" % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape))
    d = (bit_view(a).cpu() != bit_view(b).cpu()).nonzero()
    if d.numel() == 0:
        return "equal"
    i = tuple(int(v) for v in d[0])
    return "%d of %d elements differ, first at %s: %r vs %r" % (d.shape[0], a.numel(), i, a.cpu()[i].item(), b.cpu()[i].item())


def poison_(t):
    """overwrite `t` in place with the pattern no operator writes by accident: NaN for floating point, all bits set for
    integers and masks (-1; 0xFF in a uint8 or bool, which is neither False nor True)"""
    if t.is_floating_point():
        t.fill_(float("nan"))
    elif t.dtype == torch.bool:
        t.view(torch.uint8).fill_(0xFF)
    elif t.dtype == torch.uint8:
        t.fill_(0xFF)
    else:
        t.fill_(-1)
    return t


def is_poison(t):
    """every element of `t` still holds the pattern of poison_ (False for an empty tensor)"""
    if t.numel() == 0:
        return False
    if t.is_floating_point():
        return bool(torch.isnan(t).all())
    if t.dtype in (torch.bool, torch.uint8):
        return bool((bit_view(t) == 0xFF).all())
    return bool((t == -1).all())


def as_tuple(out):
    if torch.is_tensor(out) or isinstance(out, np.ndarray):
        return (out,)
    return tuple(out)


def assert_bits(got, want, what):
    got, want = as_tuple(got), as_tuple(want)
    assert len(got) == len(want), "%s: %d outputs vs %d" % (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None and w is None:
            continue
        assert g is not None and w is not None, "%s: output %d is None on one side only" % (what, i)
        assert bits_equal(g, w), "%s: output %d: %s" % (what, i, first_difference(g, w))


def replay_order(n):
    """the (value-set index, reload) sequence of check_replay for value sets 0..n-1: each in turn, the first one again, and
    the first one once more WITHOUT reloading the static inputs"""
    return [(i, True) for i in range(n)] + [(0, True), (0, False)]


# ------------------------------------------------------------------------------------------ the harness
def _to_device(values, device):
    out = []
    for v in values:
        v = as_tensor(v)
        out.append(None if v is None else v.to(device).clone())       # (clone keeps the memory format)
    return out


def _same_layout(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and a.stride() == b.stride()


def check_replay(fn, value_sets, expect=None, tol=None, between=None, eager_bits=True, device="cuda"):
    """Capture `fn(*static)` once and replay it over `value_sets` (module docstring).

    fn(*tensors) -> tensor | tuple of tensors (None entries allowed); called eagerly once on a side stream, once under
        capture, and once per replay on fresh copies of that replay's values;
    value_sets: list of input tuples (tensors, numpy arrays or None) with identical shapes, dtypes and memory formats;
    expect(values) -> the reference outputs for one value set (`values`: the tuple as given), or None;
    tol: None — `expect` is met bit for bit; otherwise tol(got, want, step) asserts closeness itself (got: the cloned
        replay outputs, on the device);
    between(): one unrelated eager call of the operator at another shape, made between two replays;
    eager_bits: the replay equals the eager call in bits (operators whose eager tests assert reproducibility).
    Returns the list of cloned outputs, one tuple per replay."""
    value_sets = [tuple(as_tensor(v) for v in vs) for vs in value_sets]
    dev = torch.device(device)
    static = _to_device(value_sets[0], dev)
    for k, vs in enumerate(value_sets):
        probe = _to_device(vs, dev)
        assert len(probe) == len(static) and all(_same_layout(a, b) for a, b in zip(probe, static)), \
            "value set %d differs from value set 0 in shape, dtype or memory format" % k

    # as GraphedTrainStep._capture: one eager run on a side stream (lazily built caches), then the capture
    cur = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        fn(*static)
    cur.wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        # detached: an output that autograd tracks as a view of a custom Function's result may be neither filled nor cloned
        captured = tuple(None if o is None else o.detach() for o in as_tuple(fn(*static)))
    torch.cuda.synchronize(dev)
    inputs = {s.untyped_storage().data_ptr() for s in static if s is not None}

    results, wanted = [], {}
    for step, (k, reload) in enumerate(replay_order(len(value_sets))):
        what = "replay %d (value set %d%s)" % (step, k, "" if reload else ", not reloaded")
        if reload:
            for dst, src in zip(static, value_sets[k]):
                if dst is not None:
                    dst.copy_(src)
        for o in captured:
            # (an output that IS an input — a gradient handed through unchanged — was just reloaded and stays as it is)
            if o is not None and o.untyped_storage().data_ptr() not in inputs:
                poison_(o)
        graph.replay()
        got = tuple(None if o is None else o.clone() for o in captured)
        torch.cuda.synchronize(dev)
        eager = tuple(None if e is None else e.detach() for e in as_tuple(fn(*_to_device(value_sets[k], dev))))
        for i, (e, c) in enumerate(zip(eager, captured)):
            assert e is None or c is None or e.data_ptr() != c.data_ptr() or e.numel() == 0, \
                "%s: output %d of an eager call IS the captured output: fn does not produce it per call" % (what, i)
        if eager_bits:
            assert_bits(got, eager, what + " against eager")
        if expect is not None:
            if k not in wanted:                 # a reference is computed once per value set and left unchanged
                wanted[k] = expect(value_sets[k])
            want = wanted[k]
            if tol is None:
                assert_bits(got, want, what + " against the reference")
            else:
                tol(got, want, what)
        results.append(got)
        if between is not None:
            between()
    return results
