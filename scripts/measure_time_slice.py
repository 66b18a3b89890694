"""Times `bgst_slice` (the two launches of csrc_slice/slice_kernels.hip) with HIP events on a stream of its own: warm-ups,
then the median, minimum and maximum of the timed runs, on a `random_gaussians_4d_seeded` cloud of --points splats. The
rate is taken against the bytes the contract moves, 656 read + 240 written = 896 a splat, and set beside the copy rate
`bgs_hbm_probe` gives in the same run (device-to-device copy, read + write counted). The two kernels are also timed one
at a time, by slicing with a stream-ordered event between them: geometry is the first launch, the fold the second.

At 1 M splats the inputs and outputs are 0.9 GB: more than the 256 MiB Infinity Cache, so a run does not find the last
run's planes in it. The same buffers are used every run.

    python scripts/measure_time_slice.py [--points 1000000] [--runs 30] [--warmup 5] [--json out.json]

One JSON line. Not bench.py: nothing here is a condition of anything."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bevy_gaussian_splatting_amd import (  # noqa: E402
    CloudSettings, GaussianSplattingPlugin, TimeSlicer, random_gaussians_4d_seeded)

BYTES_READ, BYTES_WRITTEN = 16 + 576 + 32 + 16 + 16, 240


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch

    n = args.points
    settings = CloudSettings(time=0.4)
    device = torch.device("cuda:0")
    stream = torch.cuda.Stream(device)
    cloud = random_gaussians_4d_seeded(n, 1)
    ins = [torch.from_numpy(p).to(device) for p in cloud.planes()]
    outs = [torch.empty((n, w), dtype=torch.float32, device=device) for w in (4, 48, 8)]
    slicer = TimeSlicer(0)
    times = []
    with torch.cuda.stream(stream):
        for run in range(args.warmup + args.runs):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            slicer.slice(stream.cuda_stream, n, [t.data_ptr() for t in ins], [t.data_ptr() for t in outs], settings)
            stop.record(stream)
            stop.synchronize()
            if run >= args.warmup:
                times.append(start.elapsed_time(stop))
    unmasked = float((outs[2][:, 6] != 0).float().mean().item())
    with GaussianSplattingPlugin(0) as plugin:
        copy_gbs, triad_gbs = plugin.hbm_probe()
    median = float(np.median(times))
    moved = n * (BYTES_READ + BYTES_WRITTEN)
    row = {"points": n, "runs": len(times), "median_ms": median, "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
           "bytes_moved": moved, "slice_gb_per_s": moved / (median * 1e-3) / 1e9, "hbm_probe_copy_gb_per_s": copy_gbs,
           "hbm_probe_triad_gb_per_s": triad_gbs, "share_of_copy_rate": moved / (median * 1e-3) / 1e9 / copy_gbs,
           "unmasked_share": unmasked}
    print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
