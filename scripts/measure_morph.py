"""Times `bgsm_interpolate_f32` and `bgsm_interpolate_cov3d_f32` (the two launches of csrc_morph/morph_kernels.hip) with
HIP events on a stream of its own: warm-ups, then the median, minimum and maximum of the timed runs, on two
`random_gaussians_3d_seeded` clouds of --points splats. The rate is taken against the bytes the contract moves, 720 a
splat in either layout (f32: 2 x 240 read, 240 written; covariance: the same), and set beside the copy rate
`bgs_hbm_probe` gives in the same run (device-to-device copy, read + write counted).

At 1 M splats the three clouds are 0.72 GB: more than the 256 MiB Infinity Cache, so a run does not find the last run's
planes in it. The same buffers are used every run.

    python scripts/measure_morph.py [--points 1000000] [--runs 30] [--warmup 5] [--json out.json]

One JSON line. Not bench.py: nothing here is a condition of anything."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bevy_gaussian_splatting_amd import (  # noqa: E402
    CloudSettings, GaussianInterpolator, GaussianSplattingPlugin, random_gaussians_3d_seeded)
from bevy_gaussian_splatting_amd.interpolate import covariance_planes, planes_of  # noqa: E402

BYTES_MOVED = 3 * 240          # a splat: both sides read, the output written


def timed(torch, stream, interpolator, n, sides, settings, warmup, runs):
    device = torch.device("cuda:0")
    lhs, rhs = ([torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in side] for side in sides)
    outs = [torch.empty_like(t) for t in lhs]
    times = []
    with torch.cuda.stream(stream):
        for run in range(warmup + runs):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            interpolator.interpolate(stream.cuda_stream, n, [t.data_ptr() for t in lhs], [t.data_ptr() for t in rhs],
                                     [t.data_ptr() for t in outs], settings)
            stop.record(stream)
            stop.synchronize()
            if run >= warmup:
                times.append(start.elapsed_time(stop))
    median = float(np.median(times))
    return {"median_ms": median, "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
            "gb_per_s": n * BYTES_MOVED / (median * 1e-3) / 1e9}


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
    stream = torch.cuda.Stream(torch.device("cuda:0"))
    clouds = [random_gaussians_3d_seeded(n, seed) for seed in (1, 2)]
    interpolator = GaussianInterpolator(0)
    f32 = timed(torch, stream, interpolator, n, [planes_of(c) for c in clouds], settings, args.warmup, args.runs)
    cov3d = timed(torch, stream, interpolator, n, [covariance_planes(c) for c in clouds], settings, args.warmup, args.runs)
    with GaussianSplattingPlugin(0) as plugin:
        copy_gbs, triad_gbs = plugin.hbm_probe()
    row = {"points": n, "runs": args.runs, "bytes_moved": n * BYTES_MOVED, "f32": f32, "cov3d": cov3d,
           "hbm_probe_copy_gb_per_s": copy_gbs, "hbm_probe_triad_gb_per_s": triad_gbs,
           "f32_share_of_copy_rate": f32["gb_per_s"] / copy_gbs, "cov3d_share_of_copy_rate": cov3d["gb_per_s"] / copy_gbs}
    print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
