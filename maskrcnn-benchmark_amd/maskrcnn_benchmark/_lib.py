"""ctypes binding of libdetops_gfx950.so (C ABI declared in include/detops.h).

The library is built in-tree by `make -C maskrcnn-benchmark_amd/csrc` (hipcc, gfx950) into
maskrcnn_benchmark/lib/.  There is NO fallback: if the shared object is missing or does not export
a symbol the import fails loudly — the detection-head operators exist only as HIP kernels.
"""
import ctypes
import os

import torch  # noqa: F401  — loads the HIP runtime (libamdhip64) this library links against

from . import _abi
from ._abi import SIGNATURES  # noqa: F401  — name -> (restype, argtypes), checked against the header by tests/test_abi.py

_HERE = os.path.dirname(os.path.abspath(__file__))
# DETOPS_LIB_PATH: another build of the SAME library (same ABI version, checked below) — same-box A/B measurements of a
# kernel change (tools/gpu/ab_build.sh puts the previous commit's build next to the current one)
LIB_PATH = os.environ.get("DETOPS_LIB_PATH") or os.path.join(_HERE, "lib", "libdetops_gfx950.so")


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libdetops_gfx950.so not found at %s — build it with `make -C maskrcnn-benchmark_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). The detection-head operators "
            "have no CPU / PyTorch fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    _abi.bind(lib, require_all=True)  # AttributeError if a symbol is missing: fail loudly
    if lib.detops_version(None) != _abi.ABI_VERSION:
        raise ImportError("libdetops_gfx950.so: ABI version mismatch")
    return lib


lib = _load()


def check(rc, what):
    if rc != 0:
        msg = _abi.ERRORS.get(rc, "hipError_t %d" % rc)
        raise RuntimeError("%s failed: %s" % (what, msg))


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(t):
    """The current HIP stream of the tensor's device, as an integer handle (the raw-handle query: building a
    torch.cuda.Stream object per launch costs ~5 us of host time, ~200 launches per training step)."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


DTYPE_CODE = {torch.float32: _abi.F32, torch.float16: _abi.F16, torch.bfloat16: _abi.BF16}


def tuning_set(key, value):
    """Tuning / test switch of the library (include/detops.h: detops_tuning_set)."""
    check(lib.detops_tuning_set(key.encode(), int(value)), "detops_tuning_set(%s)" % key)


def tuning_get(key):
    v = ctypes.c_int(0)
    check(lib.detops_tuning_get(key.encode(), ctypes.byref(v)), "detops_tuning_get(%s)" % key)
    return v.value
