"""The extension-operator families of tests/fuzz_cases.py (`fuzz_cases.EXTENSION`) through the product's own `_C` wrappers over
the host-emulation library (tests/cpu_shim.py backend "emu-lib"), CPU only.  tests/test_fuzz_ext_gpu.py runs the same cases,
bit for bit (tests/golden/fuzz_case_digests.json), through the same calls (tests/fuzz_ext_runs.py) on the device, on clean
and on dirtied memory.  This file is what proves the cases and their references before GPU minutes are spent, and
`test_cases_are_not_degenerate` shows from the references alone that a constant or empty output could not pass."""
import json
import os

import numpy as np
import pytest

import cpu_shim
import fuzz_cases
import fuzz_ext_runs as X

SEEDS = fuzz_cases.SEEDS
OLD_FAMILIES = ("roi_align", "nms", "deformable", "nms_batched", "roi_align_fpn", "deformable_channels_last", "focal")
# sha256 of the golden file's entries of OLD_FAMILIES (json.dumps, sorted keys) as they stood before EXTENSION was added
OLD_DIGESTS_SHA256 = "bbe9799406ce55a860b07f7c8a0061a0b4db5fb58ab692ea16323935337278af"


@pytest.fixture(autouse=True)
def _product_wrappers():
    with cpu_shim.install("emu-lib"):
        yield


def _run(family, seed):
    c = fuzz_cases.FAMILIES[family](seed)
    assert c is not None
    keep = X.RUN[family](c, X.refs(family, seed), "cpu")
    assert all(t is not None for t in keep.values())


@pytest.mark.parametrize("seed", range(SEEDS["targets_chain"]))
def test_emu_fuzz_targets_chain(seed):
    _run("targets_chain", seed)


@pytest.mark.parametrize("seed", range(SEEDS["head_losses"]))
def test_emu_fuzz_head_losses(seed):
    _run("head_losses", seed)


@pytest.mark.parametrize("seed", range(SEEDS["rpn_loss_decode"]))
def test_emu_fuzz_rpn_loss_decode(seed):
    _run("rpn_loss_decode", seed)


@pytest.mark.parametrize("seed", range(SEEDS["rpn_head_sparse"]))
def test_emu_fuzz_rpn_head_sparse(seed):
    _run("rpn_head_sparse", seed)


@pytest.mark.parametrize("seed", range(SEEDS["mask_chain"]))
def test_emu_fuzz_mask_chain(seed):
    _run("mask_chain", seed)


@pytest.mark.parametrize("seed", range(SEEDS["bbox_aug_merge"]))
def test_emu_fuzz_bbox_aug_merge(seed):
    _run("bbox_aug_merge", seed)


@pytest.mark.parametrize("seed", range(SEEDS["group_norm"]))
def test_emu_fuzz_group_norm(seed):
    _run("group_norm", seed)


@pytest.mark.parametrize("seed", range(SEEDS["bias_act"]))
def test_emu_fuzz_bias_act(seed):
    _run("bias_act", seed)


# ------------------------------------------------------------------------------------------ the sweep itself
def test_old_digests_are_unchanged_and_no_extension_case_is_none(golden_dir):
    """the digests of the seven families that tests/golden/fuzz_case_digests.json held before the extension families were
    added (sha256 of the json's entries of those families, recorded from the file as it stood): an edit that moves one is a
    bug in the edit.  Every extension case exists and is pinned."""
    import hashlib
    with open(os.path.join(golden_dir, "fuzz_case_digests.json")) as f:
        want = json.load(f)
    old = json.dumps({k: want[k] for k in OLD_FAMILIES}, sort_keys=True).encode()
    assert hashlib.sha256(old).hexdigest() == OLD_DIGESTS_SHA256
    for family in OLD_FAMILIES:
        got = [fuzz_cases.digest(fuzz_cases.FAMILIES[family](seed)) for seed in range(SEEDS[family])]
        assert got == want[family], family
    for family in fuzz_cases.EXTENSION:
        got = [fuzz_cases.digest(fuzz_cases.FAMILIES[family](seed)) for seed in range(SEEDS[family])]
        assert None not in got and len(set(got)) == len(got) and got == want[family], family



def test_every_listed_size_occurs():
    """the lists of route-changing sizes in tests/fuzz_cases.py are walked completely by each family's seeds"""
    F = fuzz_cases
    ch = [F.targets_chain(s) for s in range(SEEDS["targets_chain"])]
    assert {c["N"] for c in ch} == set(F.CHAIN_N) and {c["M"] for c in ch} == set(F.CHAIN_M)
    assert {c["K"] for c in ch} == set(F.CHAIN_K) and {c["B"] for c in ch} == set(F.CHAIN_B)
    assert {(c["hi"], c["lo"], c["lq"]) for c in ch} == set(F.CHAIN_THRESHOLDS)
    assert {(c["rpn_rule"], c["hi"]) for c in ch} == {(True, 0.7), (True, 0.5), (False, 0.7), (False, 0.5)}
    assert any(c["sampler_seed"] >> 63 for c in ch) and any(not c["sampler_seed"] >> 63 for c in ch)
    assert any(not c["gt_valid"][-1].any() for c in ch if c["N"] > 1)              # an image without a valid ground truth
    assert {c["box_valid"] is None for c in ch} == {True, False} and {c["objectness"] is None for c in ch} == {True, False}
    hl = [F.head_losses(s) for s in range(SEEDS["head_losses"])]
    assert {c["fr_R"] for c in hl} == set(F.LOSS_R) and {c["fr_C"] for c in hl} == set(F.LOSS_C)
    assert {c["mk_P"] for c in hl} == set(F.MASK_P) and {c["mk_C"] for c in hl} == set(F.MASK_C) and {c["mk_M"] for c in hl} == set(F.MASK_M)
    assert {c["kp_P"] for c in hl} == set(F.KP_P) and {c["kp_K"] for c in hl} == set(F.KP_K)
    assert {(c["kp_H"], c["kp_W"]) for c in hl} == set(F.KP_HW) and {c["kp_channels_last"] for c in hl} == {True, False}
    assert (hl[F.LOSS_ALL_UNSAMPLED]["fr_labels"] == -1).all() and not hl[F.LOSS_NO_VALID]["kp_valid"].any()
    m = hl[F.LOSS_NO_POSITIVES]
    assert not ((m["mk_labels"] > 0) & (m["mk_labels"] < m["mk_C"])).any()
    au = [F.bbox_aug_merge(s) for s in range(SEEDS["bbox_aug_merge"])]
    assert {c["C"] for c in au} == set(F.AUG_C) and {c["pass_rate"] for c in au} == set(F.AUG_PASS_RATE)
    assert {len(c["flips"]) for c in au} == {1, 2, 3, 4} and {n for c in au for per in c["rows"] for n in per} >= {0, 1, 32, 33, 129, 257, 300}
    gn = [F.group_norm(s) for s in range(SEEDS["group_norm"])]
    assert {c["G"] for c in gn} == set(F.GN_G) and {c["C"] // c["G"] for c in gn} == set(F.GN_D)
    assert {(c["H"], c["W"]) for c in gn} == set(F.GN_HW) and {c["dtype"] for c in gn} == set(F.DTYPES)
    assert any((c["H"], c["W"], c["C"] // c["G"]) == (25, 41, 2) for c in gn)       # the first plane of the split regime
    assert {(c["gamma"] is None, c["beta"] is None) for c in gn} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c["offset"] for c in gn} == {0, 1}
    rp = [F.rpn_loss_decode(s) for s in range(SEEDS["rpn_loss_decode"])]
    assert {c["A"] for c in rp} == {1, 3} and {c["N"] for c in rp} == {1, 2, 3} and {1, 8} <= {c["L"] for c in rp}
    assert not (rp[F.RPN_NOTHING_SAMPLED]["pos"] | rp[F.RPN_NOTHING_SAMPLED]["neg"]).any()
    assert not rp[F.RPN_NEGATIVES_ONLY]["pos"].any() and rp[F.RPN_NEGATIVES_ONLY]["neg"].any()
    assert {m for c in rp for (_, m, _, _) in c["decode"]} == {0, 24}
    assert any(k < c["A"] * h * w for c in rp for (k, _, _, _), (h, w) in zip(c["decode"], c["shapes"]))      # a real top-k cut
    assert any(c["N"] * min(k, c["A"] * h * w) > 256 for c in rp for (k, _, _, _), (h, w) in zip(c["decode"], c["shapes"]))
    sp = [F.rpn_head_sparse(s) for s in range(SEEDS["rpn_head_sparse"])]
    assert {c["C"] for c in sp} == set(F.SPARSE_C) and {c["rows"] for c in sp} == set(F.SPARSE_ROWS) and {c["N"] for c in sp} == {1, 2}
    assert any(c["rows"] == c["max_rows"] for c in sp) and any(c["rows"] < c["max_rows"] for c in sp)
    mc = [F.mask_chain(s) for s in range(SEEDS["mask_chain"])]
    assert {c["D"] for c in mc} == set(F.CHAIN_DETS) and {w for c in mc for _, w in c["sizes"]} == set(F.CHAIN_W)
    assert {c["M"] for c in mc} == {14, 28} and {c["padding"] for c in mc} == {1, 2} and {c["dtype"] for c in mc} == set(F.DTYPES)
    assert {c["threshold"] for c in mc} == {0.5, -1.0} and {c["n_img"] for c in mc} == {1, 2, 3}
    assert all(np.isnan(c["boxes"]).any() == (c["D"] >= 2) for c in mc)
    ba = [F.bias_act(s) for s in range(SEEDS["bias_act"])]
    assert {c["C"] for c in ba} == set(F.BIAS_C) and {c["Cs"] for c in ba} == set(F.COLSUM_C)
    assert {c["rows"] for c in ba} == {1, 63, 64, 65, 1000, 4097} and {c["dtype"] for c in ba} == set(F.DTYPES)


def test_cases_are_not_degenerate():
    """from the references alone, so that a constant or empty output could not pass: at least half the `targets_chain` cases
    contain matched, below-threshold and (where lo < hi) between-threshold boxes, sampled positives and negatives and filled
    slots; at least half the cases of each loss (box head, mask head, keypoint head, RPN) have a non-zero loss and a non-zero
    gradient; at least half the `mask_chain` cases have a detection with both set and clear pixels and a non-zero
    intersection with some ground truth; the overflow seed of `rpn_head_sparse` overflows and no other does, and at least
    half its cases have a non-zero gradient for every tensor; at least half the merges keep a candidate; every GroupNorm /
    bias case has data that a constant could not reproduce"""
    n = SEEDS["targets_chain"]
    full = 0
    for seed in range(n):
        c, r = fuzz_cases.targets_chain(seed), X.refs("targets_chain", seed)
        m = r["matched"]
        kinds = (m >= 0).any() and (m == -1).any() and (c["lo"] == c["hi"] or (m == -2).any())
        full += bool(kinds and r["pos"].any() and r["neg"].any() and r["val"].any() and np.abs(r["reg"]).max() > 0)
    assert 2 * full >= n, full
    n = SEEDS["head_losses"]
    live = {"fr": 0, "mk": 0, "kp": 0}
    for seed in range(n):
        r = X.refs("head_losses", seed)
        live["fr"] += bool(r["fr"][0] != 0 and r["fr"][1] != 0 and np.abs(r["fr"][2]).max() > 0 and np.abs(r["fr"][3]).max() > 0)
        live["mk"] += bool(r["mk"][0] != 0 and np.abs(r["mk"][1]).max() > 0)
        live["kp"] += bool(r["kp"][0] != 0 and np.abs(r["kp"][1]).max() > 0)
    assert all(2 * v >= n for v in live.values()), live
    n = SEEDS["rpn_loss_decode"]
    live = 0
    for seed in range(n):
        ro, rb, rgo, rgb = X.refs("rpn_loss_decode", seed)["ref"]
        live += bool(ro != 0 and rb != 0 and max(np.abs(g).max() for g in rgo) > 0 and max(np.abs(g).max() for g in rgb) > 0)
    assert 2 * live >= n, live
    n = SEEDS["rpn_head_sparse"]
    over = [seed for seed in range(n) if fuzz_cases.rpn_head_sparse(seed)["rows"] > fuzz_cases.rpn_head_sparse(seed)["max_rows"]]
    assert over == [fuzz_cases.SPARSE_OVERFLOW]
    c = fuzz_cases.rpn_head_sparse(fuzz_cases.SPARSE_OVERFLOW)
    assert c["rows"] == c["max_rows"] + 1 and sum(int((g != 0).any(1).sum()) for g in c["gobj"]) <= c["rows"]
    live = sum(all(float(g.abs().max()) > 0 for g in X.refs("rpn_head_sparse", seed)["grads"].values()) for seed in range(n))
    assert 2 * live >= n, live
    for seed in range(n):                      # the promised row count is the number of anchors with a non-zero gradient
        c = fuzz_cases.rpn_head_sparse(seed)
        hit = sum(int(((go != 0) | (gb.reshape(go.shape[0], go.shape[1], 4, *go.shape[2:]) != 0).any(2)).sum())
                  for go, gb in zip(c["gobj"], c["gbox"]))
        assert hit == c["rows"], (seed, hit)
    n = SEEDS["mask_chain"]
    live = 0
    for seed in range(n):
        c, r = fuzz_cases.mask_chain(seed), X.refs("mask_chain", seed)
        mixed = hit = False
        k = 0
        for planes, count in zip(c["gt_planes"], c["counts"]):
            for p in r["planes"][k:k + count]:
                p = p.numpy()
                mixed |= bool(p.any() and not p.all())
                hit |= any(bool((p & (g != 0)).any()) for g in planes)
            k += count
        live += mixed and hit
    assert 2 * live >= n, live
    n = SEEDS["bbox_aug_merge"]
    assert 2 * sum(X.refs("bbox_aug_merge", seed)["ref"][0].shape[0] > 0 for seed in range(n)) >= n
    for seed in range(SEEDS["group_norm"]):
        assert float(X.refs("group_norm", seed)["x"].float().abs().max()) > 0
    for seed in range(SEEDS["bias_act"]):
        r = X.refs("bias_act", seed)
        assert r["x"].numel() <= 4 or float(r["x"].float().std()) > 0
