"""Generate tests/golden/ref_cpu_live.npz: what the reference's own CPU kernels (oracle/_ref, compiled in place by
oracle/build_ref.py) return for the inputs of the tests that otherwise need those kernels at run time, so that the
tests also run where the reference tree is absent.  Build container only; re-run with
    python tests/golden/make_golden_ref_live.py

  live_ra_out_<i>, live_nms_keep      test_oracle.py::test_live_compiled_reference_if_present
  adj_<case>_lhs, adj_<case>_abs,     test_oracle.py::test_roi_align_backward_is_the_adjoint_of_the_compiled_reference_forward:
  adj_<case>_idx, adj_<case>_d        <forward(x), g> and sum |forward(x) * g| in fp64, and <forward(x + e_idx) - forward(x), g>
                                      for the 5 drawn elements (whether the test uses them or not)
  f64_ra_sha256_<i>, f64_nms_keep_<t> test_cpu_branch.py::test_cpu_branch_float64_is_bit_equal_to_the_compiled_reference:
                                      SHA-256 of the float64 ROIAlign outputs' bytes (bit equality), the kept NMS indices
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import oracle  # noqa: E402
import synth  # noqa: E402
from oracle import build_ref  # noqa: E402

LIVE_CFGS = [(7, 7, 2), (2, 9, 0)]
F64_CFGS = [(7, 7, 2), (3, 5, 0), (14, 14, 2)]
F64_NMS_THRESHOLDS = (0.3, 0.7)


def adjoint_inputs(case):
    """the adjoint test's inputs: (rng after drawing them, input map, rois, scale, pooled size)"""
    rng = np.random.RandomState(17)
    if case == "cfg1":
        inp, rois, scale = synth.cfg1_roi_align(seed=9, K=512, C=256)
        return rng, inp, rois, scale, 7
    h, w = synth.fpn_shapes()[1]
    inp = rng.randn(2, 32, h, w).astype(np.float32)
    all_rois = synth.fpn_rois(seed=3, per_image=300, n_images=2)
    rois = all_rois[synth.level_map(all_rois) == 1]
    return rng, inp, rois, 1.0 / 8, 14


def f64_inputs():
    """the float64 test's inputs: values that are NOT float32-representable (seeded noise on the cfg-1 map)"""
    inp, rois, scale = synth.cfg1_roi_align(seed=4, K=60, C=7)
    x, r = torch.from_numpy(inp).double(), torch.from_numpy(rois).double()
    x = x + torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(4)) * 1e-9
    bx, sc = synth.nms_boxes(800, seed=2)
    return x, r, scale, torch.from_numpy(bx).double() + 1e-7, torch.from_numpy(sc).double()


def main():
    build_ref.build()
    ref = oracle.ref()
    assert ref is not None, "build oracle/_ref first (needs the reference tree)"
    out = {}
    inp, rois, scale = synth.cfg1_roi_align(seed=21, K=40, C=5)
    for i, (ph, pw, sr) in enumerate(LIVE_CFGS):
        out["live_ra_out_%d" % i] = ref.roi_align_forward(torch.from_numpy(inp), torch.from_numpy(rois), scale, ph, pw, sr).numpy()
    b, s = synth.nms_boxes(700, seed=33)
    out["live_nms_keep"] = ref.nms(torch.from_numpy(b), torch.from_numpy(s), 0.6).numpy().astype(np.int64)

    for case in ("cfg1", "fpn-level"):
        rng, inp, rois, scale, p = adjoint_inputs(case)
        fwd = lambda x: ref.roi_align_forward(torch.from_numpy(x), torch.from_numpy(rois), scale, p, p, 2).numpy()  # noqa: E731
        y = fwd(inp)
        g = rng.randn(*y.shape).astype(np.float32)
        idx, d = [], []
        for _ in range(5):
            ix = tuple(rng.randint(0, n) for n in inp.shape)
            x2 = inp.copy()
            x2[ix] += 1.0
            idx.append(ix)
            d.append(float(((fwd(x2).astype(np.float64) - y.astype(np.float64)) * g).sum()))
        out["adj_%s_lhs" % case] = np.float64((y.astype(np.float64) * g.astype(np.float64)).sum())
        out["adj_%s_abs" % case] = np.float64(np.abs(y.astype(np.float64) * g).sum())
        out["adj_%s_idx" % case] = np.asarray(idx, np.int64)
        out["adj_%s_d" % case] = np.asarray(d, np.float64)

    x, r, scale, tb, ts = f64_inputs()
    for i, (ph, pw, sr) in enumerate(F64_CFGS):
        out["f64_ra_sha256_%d" % i] = np.asarray(hashlib.sha256(ref.roi_align_forward(x, r, scale, ph, pw, sr).numpy().tobytes()).hexdigest())
    for thr in F64_NMS_THRESHOLDS:
        out["f64_nms_keep_%d" % int(thr * 100)] = ref.nms(tb, ts, thr).numpy().astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "ref_cpu_live.npz"), **out)
    print("ref_cpu_live.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
