"""bench.py's launch logic without a GPU: `--gpus N` must produce N ranks by itself (the reference is started with
`python -m torch.distributed.launch --nproc_per_node=$NGPUS tools/train_net.py`, README.md:147-163, process-group init at
tools/train_net.py:158-166), must refuse a world size that differs from --gpus, and the timed region / max-over-ranks /
one-JSON-line plumbing must work over a real 2-rank process group (gloo here; RCCL on the GPU node)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    env.update(extra)
    return env


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line, from rank 0: %r" % (stdout,)
    return json.loads(lines[0])


def test_gpus_2_launches_two_ranks_by_itself():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "4", "--warmup", "1", "--stub-step"],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2
    assert line["ranks_seen_by_allreduce"] == 2.0      # the collective really spanned two processes
    assert line["steps"] == 4 and line["warmup"] == 1 and line["stub"] is True
    assert "launching 2 ranks" in r.stderr


def test_driver_style_launch_is_not_relaunched():
    """Under torch.distributed.run (WORLD_SIZE set) bench.py is a rank: it must not spawn again."""
    sys.path.insert(0, ROOT)
    import bench
    cmd = bench.self_launch_command(["--gpus", "2", "--steps", "3", "--warmup", "0", "--stub-step"], 2)
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and "127.0.0.1" in cmd
    r = subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _json_line(r.stdout)["rccl_ranks"] == 2
    assert "launching" not in r.stderr


def test_world_size_mismatch_fails_loudly():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--stub-step"], env=_env(WORLD_SIZE="1", RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 2 but WORLD_SIZE=1" in (r.stderr + r.stdout)
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--stub-step"],
                       env=_env(WORLD_SIZE="2", RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 1 but WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_steps_set_the_timed_steps_and_dump_outputs_writes_the_last_one(tmp_path):
    """--steps K runs exactly K timed steps (ms_per_step = the region / K); --dump-outputs writes the last timed step's result,
    the same file in every run with the same arguments; --steps below 1 is refused"""
    dumps = []
    for run in range(2):
        d = tmp_path / ("run%d" % run)
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--stub-step",
                            "--dump-outputs", str(d)], env=_env(), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = _json_line(r.stdout)
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert sorted(os.listdir(d)) == ["ranks_seen.npy"]
        dumps.append(np.load(d / "ranks_seen.npy"))
    assert dumps[0].dtype == np.float32 and dumps[0].tolist() == [1.0]
    assert np.array_equal(dumps[0], dumps[1])
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0", "--stub-step"], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


def test_step_outputs_samples_parameters_at_fixed_indices(tmp_path):
    """bench.py::step_outputs: the losses whole, every trainable parameter whole up to PARAM_SAMPLE elements and sampled at
    the same indices in every call above that, frozen parameters left out; dump_outputs refuses more than DUMP_MAX_BYTES"""
    torch = pytest.importorskip("torch")
    sys.path.insert(0, ROOT)
    import bench
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(100, 100), torch.nn.Linear(100, 3))
    model[1].bias.requires_grad_(False)
    losses = {"loss_a": torch.tensor(0.5), "loss_b": torch.tensor(1.25, dtype=torch.float64)}
    out = bench.step_outputs(losses, model)
    assert sorted(out) == ["loss_a", "loss_b", "param.0.bias", "param.0.weight", "param.1.weight"]
    assert out["loss_a"].dtype == np.float32 and out["loss_b"].dtype == np.float64
    assert out["param.0.weight"].shape == (bench.PARAM_SAMPLE,) and out["param.0.weight"].dtype == np.float32
    assert np.array_equal(out["param.1.weight"], model[1].weight.detach().reshape(-1).numpy())
    assert np.isin(out["param.0.weight"], model[0].weight.detach().numpy()).all()
    again = bench.step_outputs(losses, model)
    assert all(np.array_equal(out[k], again[k]) for k in out)
    assert bench.dump_outputs(str(tmp_path), out) == len(out)
    assert np.array_equal(np.load(tmp_path / "param.0.weight.npy"), out["param.0.weight"])
    with pytest.raises(SystemExit, match="limit"):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_MAX_BYTES // 4 + 1, np.float32)})


def test_shipped_miopen_db_from_a_read_only_checkout_is_copied_writable(tmp_path, monkeypatch):
    """bench.py::setup_miopen_db: MIOpen writes lock files, journals and records beside the databases it is pointed at, so the
    scratch copy of the shipped database must be writable even when the checkout is read-only (modes are not copied)"""
    import stat
    import tempfile
    sys.path.insert(0, ROOT)
    import bench
    root = tmp_path / "checkout"
    shipped = root / "maskrcnn-benchmark_amd" / "miopen_db"
    (shipped / "db").mkdir(parents=True)
    (shipped / "cache").mkdir()
    (shipped / "db" / "gfx950100.HIP.udb.txt").write_text("key=solver:params\n")
    (shipped / "cache" / "gfx950100.ukdb").write_bytes(b"SQLite format 3\0")
    for d, dirs, files in os.walk(root, topdown=False):
        for f in files:
            os.chmod(os.path.join(d, f), 0o444)
        os.chmod(d, 0o555)
    scratch = tmp_path / "tmp"
    scratch.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(root))
    monkeypatch.setattr(tempfile, "tempdir", str(scratch))
    monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    monkeypatch.delenv("MIOPEN_CUSTOM_CACHE_DIR", raising=False)
    try:
        assert bench.setup_miopen_db(None) == "shipped:" + str(shipped)
        db, cache = os.environ["MIOPEN_USER_DB_PATH"], os.environ["MIOPEN_CUSTOM_CACHE_DIR"]
        assert db.startswith(str(scratch)) and cache.startswith(str(scratch))
        assert open(os.path.join(db, "gfx950100.HIP.udb.txt")).read() == "key=solver:params\n"
        assert open(os.path.join(cache, "gfx950100.ukdb"), "rb").read() == b"SQLite format 3\0"
        for p in (db, cache, os.path.join(db, "gfx950100.HIP.udb.txt"), os.path.join(cache, "gfx950100.ukdb")):
            assert os.stat(p).st_mode & stat.S_IWUSR, p
    finally:
        for d, dirs, files in os.walk(root):
            os.chmod(d, 0o755)


def test_hw_queue_pin_and_sampling_cap():
    sys.path.insert(0, ROOT)
    import bench
    old = os.environ.pop("GPU_MAX_HW_QUEUES", None)
    try:
        assert bench.pin_hip_queues() == bench.HW_QUEUES_DEFAULT == os.environ["GPU_MAX_HW_QUEUES"]
        os.environ["GPU_MAX_HW_QUEUES"] = "1"
        assert bench.pin_hip_queues() == "1"      # an explicit setting wins
    finally:
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
        if old is not None:
            os.environ["GPU_MAX_HW_QUEUES"] = old
    pytest.importorskip("torch")
    sys.path.insert(0, os.path.join(ROOT, "maskrcnn-benchmark_amd"))
    from maskrcnn_benchmark._C import KernelTimer, _NOSPAN
    t = KernelTimer(every_cap=2)
    import torch
    x = torch.zeros(1)
    # a name sampled every 8th call is sampled every 2nd under the cap: 20 calls -> 10 spans (>= 10 event pairs at
    # the driver's --steps 20)
    spans = [t.span("frozen_bn_fwd", x, every=8) for _ in range(20)]
    assert sum(s is not _NOSPAN for s in spans) == 10


def test_kernel_timer_per_name_strides_from_a_counted_step():
    """bench.py's sampling plan: a counting pass (no events) over one warm-up step gives calls per step per entry point; the
    timed region then samples every name with stride calls x steps / 12 -> >= 10 event pairs per name, few more."""
    pytest.importorskip("torch")
    sys.path.insert(0, os.path.join(ROOT, "maskrcnn-benchmark_amd"))
    import torch
    from maskrcnn_benchmark._C import KernelTimer, _NOSPAN
    x = torch.zeros(1)
    counter = KernelTimer(count_only=True)
    per_step = {"frozen_bn_fwd[a]": 13, "roi_align_fpn_fwd[b]": 1, "frozen_bn_bwd[c]": 3}
    for name, n in per_step.items():
        assert all(counter.span(name, x, every=8) is _NOSPAN for _ in range(n))
    steps = 20
    strides = {name: max(1, (n * steps) // 12) for name, n in counter.calls.items()}
    timer = KernelTimer(every_cap=2, strides=strides)
    sampled = {name: sum(timer.span(name, x, every=8) is not _NOSPAN for _ in range(n * steps)) for name, n in per_step.items()}
    assert all(10 <= v <= 24 for v in sampled.values()), sampled
    assert sum(sampled.values()) < sum(per_step.values()) * steps / 4      # far fewer than "every 2nd call of everything"


def test_prewarm_visits_every_mask_head_batch_size_once():
    """bench.py::prewarm_mask_batch_sizes: one untimed step per possible mask-head batch size (total slots from one granule per
    image to the quota per image in steps of one granule), every image within its quota, the mode restored afterwards"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "maskrcnn-benchmark_amd"))
    import bench
    from maskrcnn_benchmark.modeling.roi_heads.mask_head import mask_head as mh

    class Head(object):
        max_positives, last_slots = 128, None

    class Model(object):
        roi_heads = {"mask": Head()}

    seen = []
    old = mh.SLOT_MODE
    mh.SLOT_MODE = "dynamic"
    try:
        for n in (1, 2, 3):
            seen.clear()
            done = bench.prewarm_mask_batch_sizes(Model(), lambda *b: seen.append([int(v) for v in mh.SLOT_MODE.split(",")]),
                                                  [("images", "targets")], n)
            g = mh.SLOT_GRANULE
            assert done == len(seen) == (n * 128 - n * g) // g + 1
            assert [sum(s) for s in seen] == list(range(n * g, n * 128 + 1, g))
            assert all(len(s) == n and all(g <= v <= 128 and v % g == 0 for v in s) for s in seen)
            assert mh.SLOT_MODE == "dynamic"
        mh.SLOT_MODE = "fixed"
        assert bench.prewarm_mask_batch_sizes(Model(), lambda *b: seen.append(1), [("i", "t")], 2) == 0
    finally:
        mh.SLOT_MODE = old
