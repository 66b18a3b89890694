"""Times one playback step, from a changed `time` to a resident cloud that is ready to render, for the time slice of a 4D
cloud and for the f32 morph between two clouds, at --points splats. A step frees the previous step's cloud and makes the
next one. It is timed twice over: by two HIP events on `bgs_stream` around the whole step (the second is recorded
after the step's last call has returned, so host time between the calls is inside), and by the host's clock. Warm-up
steps, then --steps timed ones; the whole series --repeats times in one process, which gives the run-to-run spread.

    --route api        what a caller of `plugin.slice_4d(cloud4d, settings)` and `MorphPair.at(settings)` gets in the tree the
                       script runs in. Run in a checkout of the commit before the device hand-off this is the baseline:
                       planes downloaded and uploaded again, and `slice_4d` putting the five planes up on every call.
    --route resident   `ResidentCloud4d.at` and `MorphPair.at` over device planes, and the step's split: produce (the
                       kernel alone, events), the upload as a whole (host clock), of which allocate is estimated by
                       timing `bgs_device_alloc` of the cloud's two buffers' sizes (the same hipMalloc), and the
                       `bgs_cloud_free` of the previous cloud (host clock). Copy, pack and the synchronisation at the
                       end of the upload happen inside one library call and are reported together, as the upload less
                       the allocation.

    python scripts/measure_hand_off.py --route resident [--points 1000000] [--steps 20] [--warmup 5] [--repeats 3] [--json out.json]

One JSON line. Not bench.py: nothing here is a condition of anything."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bevy_gaussian_splatting_amd import (  # noqa: E402
    CloudSettings, GaussianSplattingPlugin, random_gaussians_3d_seeded, random_gaussians_4d_seeded)


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def series(torch, plugin, step, warmup, steps, repeats):
    """`step(k, previous_handle) -> handle` run warmup + steps times a repeat. Returns the events' and the clock's times."""
    out = []
    for _ in range(repeats):
        ev_ms, wall_ms, handle = [], [], None
        for k in range(warmup + steps):
            stream = torch.cuda.ExternalStream(plugin.stream_handle())
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            start.record(stream)
            handle = step(k, handle)
            stop.record(torch.cuda.ExternalStream(plugin.stream_handle()))
            stop.synchronize()
            t1 = time.perf_counter()
            if k >= warmup:
                ev_ms.append(start.elapsed_time(stop))
                wall_ms.append((t1 - t0) * 1e3)
        handle.free()
        out.append({"events": summary(ev_ms), "host_clock": summary(wall_ms)})
    medians = [r["events"]["median_ms"] for r in out]
    return {"repeats": out, "median_of_medians_ms": float(np.median(medians)),
            "spread_of_medians": float((max(medians) - min(medians)) / np.median(medians))}


def time_of(k, count):
    return 0.1 + 0.8 * ((k * 7) % count) / count           # a new time every step


def clock(fn):
    t0 = time.perf_counter()
    result = fn()
    return result, (time.perf_counter() - t0) * 1e3


def split(torch, plugin, produce, upload, n, warmup, steps):
    """The resident step in parts. `produce()` enqueues the kernel on bgs_stream, `upload()` returns the handle."""
    parts = {"produce_ms": [], "upload_ms": [], "allocate_ms": [], "free_previous_ms": []}
    handle = None
    for k in range(warmup + steps):
        stream = torch.cuda.ExternalStream(plugin.stream_handle())
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        produce(k)
        stop.record(stream)
        stop.synchronize()
        (a, b), alloc_ms = clock(lambda: (plugin.device_alloc(n * 16), plugin.device_alloc(n * 256)))
        plugin.device_free(a)
        plugin.device_free(b)
        _, free_ms = clock(handle.free) if handle is not None else (None, 0.0)
        handle, upload_ms = clock(upload)
        if k >= warmup:
            parts["produce_ms"].append(start.elapsed_time(stop))
            parts["upload_ms"].append(upload_ms)
            parts["allocate_ms"].append(alloc_ms)
            parts["free_previous_ms"].append(free_ms)
    handle.free()
    row = {name: summary(v) for name, v in parts.items()}
    row["copy_pack_synchronise_ms"] = {"median_ms": row["upload_ms"]["median_ms"] - row["allocate_ms"]["median_ms"]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("api", "resident"), required=True)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch

    n, count = args.points, args.warmup + args.steps
    cloud4d = random_gaussians_4d_seeded(n, 3)
    lhs, rhs = random_gaussians_3d_seeded(n, 1), random_gaussians_3d_seeded(n, 2)
    row = {"route": args.route, "points": n, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    with GaussianSplattingPlugin(0) as plugin:
        row["build_id"] = plugin.build_id()

        def free(previous):
            if previous is not None:
                previous.free()

        with plugin.morph_pair(lhs, rhs) as pair:
            def morph_step(k, previous):
                free(previous)
                return pair.at(CloudSettings(time=time_of(k, count)))
            row["morph_f32"] = series(torch, plugin, morph_step, args.warmup, args.steps, args.repeats)
            if args.route == "resident":
                row["morph_f32"]["split"] = split(
                    torch, plugin,
                    lambda k: pair.enqueue(plugin.stream_handle(), CloudSettings(time=time_of(k, count))),
                    lambda: plugin.upload_device_planes("f32", n, pair.out_ptrs), n, args.warmup, args.steps)
        if args.route == "api":
            def slice_step(k, previous):
                free(previous)
                return plugin.slice_4d(cloud4d, CloudSettings(time=time_of(k, count)))
            row["slice"] = series(torch, plugin, slice_step, args.warmup, args.steps, args.repeats)
        else:
            with plugin.resident_4d(cloud4d) as resident:
                def slice_step(k, previous):
                    free(previous)
                    return resident.at(CloudSettings(time=time_of(k, count)))
                row["slice"] = series(torch, plugin, slice_step, args.warmup, args.steps, args.repeats)
                row["slice"]["split"] = split(
                    torch, plugin,
                    lambda k: resident.enqueue(plugin.stream_handle(), CloudSettings(time=time_of(k, count))),
                    lambda: plugin.upload_device_planes("cov3d", n, resident.out_ptrs), n, args.warmup, args.steps)
            # the one-shot wrapper in this tree, for the record: it still puts the five planes up on every call
            def one_shot_step(k, previous):
                free(previous)
                return plugin.slice_4d(cloud4d, CloudSettings(time=time_of(k, count)))
            row["slice_one_shot"] = series(torch, plugin, one_shot_step, 2, 5, 1)
    print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
