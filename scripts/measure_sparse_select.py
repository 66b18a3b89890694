"""Times `bgss_neighbor_counts` (the two memsets and the four launches of csrc_sparse/sparse_kernels.hip) with HIP events
on a stream of its own: warm-ups, then the median, minimum and maximum of the timed runs. Two clouds of --points splats at
the reference's radius 0.05: its own distribution, U(-20, 20)^3, where nearly every splat is sparse, and the trained-like
cloud of `trained_like_gaussians_3d_seeded`, whose splats lie on surfaces. Each with cap 0 and cap 3. Also printed: the
table size the library chooses, the heaviest cell (counted on the host by the rule of sparse_math.h), the share of sparse
splats, and, if scipy imports, the host time of a cKDTree count of the same points.

    python scripts/measure_sparse_select.py [--points 1000000] [--runs 30] [--warmup 5] [--json out.json]

One JSON line per (cloud, cap). Not bench.py: nothing here is a condition of anything."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bevy_gaussian_splatting_amd import (  # noqa: E402
    SparseGrid, SparseSelect, random_gaussians_3d_seeded, trained_like_gaussians_3d_seeded)


def heaviest_cell(points, radius):
    """(points in the fullest cell, cells in use) under cell_scale / cell_of of sparse_math.h (no clamp is reached here)."""
    scale = 1.0 / (float(np.float32(radius)) * (1.0 + 1.0 / 1024.0))
    c = np.floor(points[:, :3].astype(np.float64) * scale).astype(np.int64) + (1 << 20)
    keys = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, counts = np.unique(keys, return_counts=True)
    return int(counts.max()), int(len(counts))


def table_bits(n):
    bits = 6
    while bits < 26 and (1 << bits) < 2 * n:
        bits += 1
    return bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-kdtree", action="store_true")
    args = ap.parse_args()
    import torch

    select = SparseSelect()
    n = args.points
    device = torch.device("cuda:0")
    stream = torch.cuda.Stream(device)
    rows = []
    with SparseGrid(n, 0) as grid:
        for name, make in (("reference U(-20,20)^3", random_gaussians_3d_seeded), ("trained-like", trained_like_gaussians_3d_seeded)):
            pv = np.ascontiguousarray(make(n, 1).position_visibility)
            heavy, cells = heaviest_cell(pv, select.radius)
            points = torch.from_numpy(pv).to(device)
            counts = torch.empty(n, dtype=torch.int32, device=device)
            kd_ms = None
            if not args.no_kdtree:
                try:
                    from scipy.spatial import cKDTree
                    t0 = time.perf_counter()
                    tree = cKDTree(pv[:, :3].astype(np.float64))
                    kd = tree.query_ball_point(pv[:, :3].astype(np.float64), select.radius, return_length=True, workers=-1)
                    kd_ms = 1e3 * (time.perf_counter() - t0)
                    del tree, kd
                except ImportError:
                    pass
            for cap in (0, select.neighbor_threshold):
                times = []
                with torch.cuda.stream(stream):
                    for run in range(args.warmup + args.runs):
                        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        start.record(stream)
                        grid.neighbor_counts(stream.cuda_stream, points.data_ptr(), n, select.radius, counts.data_ptr(), cap=cap)
                        stop.record(stream)
                        stop.synchronize()
                        if run >= args.warmup:
                            times.append(start.elapsed_time(stop))
                got = counts.cpu().numpy().view(np.uint32)
                row = {"cloud": name, "points": n, "radius": select.radius, "cap": cap, "runs": len(times),
                       "median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
                       "table_slots": 1 << table_bits(n), "cells_in_use": cells, "heaviest_cell": heavy,
                       "sparse_share": float((got < select.neighbor_threshold).mean()), "max_count": int(got.max()),
                       "ckdtree_build_and_count_ms_all_host_threads": kd_ms}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
