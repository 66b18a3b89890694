"""Times the reduction behind `BGS_BOUNDS_CLOUD` (csrc/bounds_kernels.hip) on the position planes of the 1 M-splat f32
cloud and the 5 M-splat f16 cloud (the plane is f32, 16 bytes a splat, in every cloud format: the format does not reach
the kernel) and sets its read rate beside the copy rate `bgs_hbm_probe` gives in the same run.

libbgs has no entry point that runs the reduction alone, so the timing is taken by a program of its own,
scripts/micro/cloud_bounds_time.hip, which compiles the kernel file as it stands: HIP events on a stream of its own,
warm-ups, then the median, minimum and maximum of the timed runs, the plane resident in enough copies that no run finds
it in the 256 MiB Infinity Cache. This script builds the program when it is missing or older than its sources, runs it
once a cloud, and adds the probe's figures. The reduction reads 16 bytes a splat and writes 24 bytes in all; the probe's
copy figure counts bytes read plus bytes written, so the two are rates of the same memory system.

    python scripts/measure_cloud_bounds.py [--points 1000000 5000000] [--runs 30] [--warmup 5] [--json out.json]

One JSON line. Not bench.py: nothing here is a condition of anything."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bevy_gaussian_splatting_amd import GaussianSplattingPlugin  # noqa: E402

CSRC = os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc")
SOURCE = os.path.join(ROOT, "scripts", "micro", "cloud_bounds_time.hip")
PROGRAM = os.path.join(ROOT, "scripts", "micro", "cloud_bounds_time")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# (the library's flags, csrc/Makefile)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function"]


def build():
    deps = [SOURCE] + [os.path.join(CSRC, f) for f in ("bounds_kernels.hip", "bounds_math.h", "kernels.h", "frame_params.h", "bgs_device.h")]
    if not os.path.exists(PROGRAM) or any(os.path.getmtime(d) > os.path.getmtime(PROGRAM) for d in deps):
        subprocess.run([HIPCC, *FLAGS, SOURCE, "-o", PROGRAM], check=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    build()
    rows = []
    for n in args.points:
        out = subprocess.run([PROGRAM, str(n), str(args.runs), str(args.warmup)], check=True, capture_output=True, text=True, timeout=600).stdout
        rows.append(json.loads(out.strip().splitlines()[-1]))
    with GaussianSplattingPlugin(0) as plugin:
        copy_gbs, triad_gbs = plugin.hbm_probe()
    for row in rows:
        row["reduce_share_of_copy_rate"] = row["reduce"]["gb_per_s"] / copy_gbs
        row["refresh_share_of_copy_rate"] = row["refresh"]["gb_per_s"] / copy_gbs
    result = {"clouds": rows, "hbm_probe_copy_gb_per_s": copy_gbs, "hbm_probe_triad_gb_per_s": triad_gbs}
    print(json.dumps(result), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
