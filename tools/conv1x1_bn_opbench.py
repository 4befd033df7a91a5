"""Per-shape timing of the fused 1x1 convolution + FrozenBN launch (csrc/conv1x1_bn.hip) against what it replaces:
MIOpen's convolution followed by the FrozenBN launch.  The shapes are the 16 distinct (C, K, stride, residual, ReLU) cases of
the R-50 backbone's bottlenecks at the benchmark's image size (800 x 1344 padded), at the benchmark's 2 images per GPU and at
1 image (half the rows); every case runs under both tile configurations.  The routing table of csrc/conv1x1_bn.hip is
filled from this tool's output (profiles/conv1x1_bn_opbench.txt).

    python tools/conv1x1_bn_opbench.py [--rounds 5] [--iters 20] [--out FILE]

Device time: `iters` launches are enqueued behind a long matrix product, so the events around them see the kernels back
to back without the host's enqueue time; `rounds` rounds with the variants alternating inside a round, the median round
per variant.  Host time: the wall clock of the same enqueue loop, per call.  MIOpen reads the shipped tuning database, as
bench.py does."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "maskrcnn-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (C, K, stride, input H, input W, residual, relu) at 2 x 3 x 800 x 1344: res2 200 x 336 ... res5 25 x 42
SHAPES = [
    (64, 64, 1, 200, 336, 0, 1), (64, 256, 1, 200, 336, 1, 1), (64, 256, 1, 200, 336, 0, 0), (256, 64, 1, 200, 336, 0, 1),
    (256, 128, 2, 200, 336, 0, 1), (128, 512, 1, 100, 168, 1, 1), (256, 512, 2, 200, 336, 0, 0), (512, 128, 1, 100, 168, 0, 1),
    (512, 256, 2, 100, 168, 0, 1), (256, 1024, 1, 50, 84, 1, 1), (512, 1024, 2, 100, 168, 0, 0), (1024, 256, 1, 50, 84, 0, 1),
    (1024, 512, 2, 50, 84, 0, 1), (512, 2048, 1, 25, 42, 1, 1), (1024, 2048, 2, 50, 84, 0, 0), (2048, 512, 1, 25, 42, 0, 1),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    bench.setup_miopen_db()
    import torch
    import torch.nn.functional as F
    from maskrcnn_benchmark import _C

    dev = torch.device("cuda:0")
    cl = torch.channels_last
    lines = ["# %s; median of %d rounds of %d launches, us per call: device time | host enqueue time" % (
                 torch.cuda.get_device_name(0), args.rounds, args.iters),
             "# pair = MIOpen convolution + frozen_bn_act_forward (two launches); t32 / t16 = the fused launch, config 1 / 2",
             "%5s %5s %2s %7s %3s %4s | %7s %7s %7s | %7s %7s %7s | %s" % (
                 "C", "K", "s", "rows", "res", "relu", "pair", "t32", "t16", "pair", "t32", "t16", "best")]
    big = torch.randn(6144, 6144, device=dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    for N in (2, 1):
        for C, K, s, H, W, res, relu in SHAPES:
            x = torch.randn(N, C, H, W, generator=g).to(dev).contiguous(memory_format=cl)
            w = (torch.randn(K, C, 1, 1, generator=g) * (2.0 / C) ** 0.5).to(dev)
            scale = (torch.rand(K, generator=g) + 0.5).to(dev)
            bias = torch.randn(K, generator=g).to(dev)
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            r = torch.randn(N, K, Ho, Wo, generator=g).to(dev).contiguous(memory_format=cl) if res else None

            def pair():
                return _C.frozen_bn_act_forward(F.conv2d(x, w, None, s), scale, bias, r, relu)

            variants = {"pair": pair}
            for name, cfg in (("t32", 1), ("t16", 2)):
                if _C.conv1x1_bn_config(x, w, s, r, cfg) == cfg:
                    variants[name] = (lambda cfg=cfg: _C.conv1x1_bn_forward(x, w, scale, bias, r, relu, s, cfg))
            ref = pair()
            for name, fn in variants.items():
                for _ in range(3):
                    out = fn()
                err = (out - ref).abs().max().item()
                assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (name, C, K, s, err)
            times = {name: [] for name in variants}
            host = {name: [] for name in variants}
            for _ in range(args.rounds):
                for name, fn in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    torch.mm(big, big)
                    torch.mm(big, big)
                    a.record()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        fn()
                    host[name].append((time.perf_counter() - t0) * 1e6 / args.iters)
                    b.record()
                    b.synchronize()
                    times[name].append(a.elapsed_time(b) * 1e3 / args.iters)
            med = {name: statistics.median(t) for name, t in times.items()}
            hmed = {name: statistics.median(t) for name, t in host.items()}
            best = min(med, key=med.get)
            cell = lambda d, k: "%.1f" % d[k] if k in d else "-"  # noqa: E731
            lines.append("%5d %5d %2d %7d %3d %4d | %7s %7s %7s | %7s %7s %7s | %s" % (
                C, K, s, N * Ho * Wo, res, relu, cell(med, "pair"), cell(med, "t32"), cell(med, "t16"),
                cell(hmed, "pair"), cell(hmed, "t32"), cell(hmed, "t16"), best))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
