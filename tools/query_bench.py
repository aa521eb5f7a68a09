#!/usr/bin/env python3
"""Ray queries against the AOV launch they share their walk with: C3 (4096^2, 1000 spheres),
every buffer in device memory, one stream.

  (a) aov        rt_render_aov_device, depth + object, tuning cam = 0: the tree walk from rays the kernel builds
                 from the pixel (4 + 4 B of stores per ray)
  (b) nearest    rt_query_nearest_device, t + object, on exactly those camera rays: built on the host with numpy
                 from the camera matrix (main.rs:39-41, 50-53, camera.rs:78) and uploaded once, outside the timed
                 region (48 B of loads and 8 + 4 B of stores per ray)
  (c) permuted   the same rays in a fixed random permutation: the price of incoherent rays (reported, not fixed)
  (d) occluded   rt_query_occluded_device without a range on (b)'s rays (48 B of loads, 1 B of stores)
One warm-up per case, then the cases alternated in rounds in this one process; each times a batch of launches
between two device events, until each case has run for about --seconds.  The figure per case is the median over
rounds of the time per launch; the rounds are kept.  (b)'s answers are compared with (a)'s buffers before anything
is timed.  One JSON line goes to --out (under profiles/).  No step is tried twice.

    python tools/query_bench.py
    python tools/query_bench.py --side 1024
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rust-raytrace_amd")]


def camera_rays(np, cam, side):
    """The centre-jitter camera rays of a side x side frame, row-major [side * side, 6] float64: main.rs:39-41,
    50-53, then matrix * (px, py, 1) normalised component by component (camera.rs:78)."""
    pos = [float(v) for v in cam.position]
    m = [float(v) for v in cam.matrix]
    hw = hh = float(side) / 2.0
    scale = max(1.0 / hw, 1.0 / hh)
    px = ((np.arange(side, dtype=np.float64) + 0.5) - hw) * scale
    py = ((np.arange(side, dtype=np.float64) + 0.5) - hh) * scale
    px, py = np.broadcast_to(px[None, :], (side, side)), np.broadcast_to(py[:, None], (side, side))
    vx = m[0] * px + m[1] * py + m[2] * 1.0
    vy = m[3] * px + m[4] * py + m[5] * 1.0
    vz = m[6] * px + m[7] * py + m[8] * 1.0
    n = np.sqrt(vx * vx + vy * vy + vz * vz)
    rays = np.empty((side * side, 6), np.float64)
    rays[:, 0], rays[:, 1], rays[:, 2] = pos
    rays[:, 3], rays[:, 4], rays[:, 5] = (vx / n).reshape(-1), (vy / n).reshape(-1), (vz / n).reshape(-1)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--spheres", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device time per case")
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch                     # first: the process then uses torch's HIP runtime for both
    import libraytrace as lr
    from libraytrace import scenes

    side = args.side
    n = side * side
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    spec = scenes.config3(side, side, n=args.spheres)
    scene = lr.Scene.deserialize(spec.to_text())
    host_rays = camera_rays(np, scene.desc().camera, side)
    with torch.cuda.stream(stream):
        d_rays = torch.from_numpy(host_rays).to(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(12345)
        perm = torch.randperm(n, device=dev, generator=gen)
        d_perm_rays = d_rays[perm].contiguous()
    depth = torch.zeros((side, side), dtype=torch.float32, device=dev)
    aobj = torch.zeros((side, side), dtype=torch.int32, device=dev)
    t = torch.zeros(n, dtype=torch.float64, device=dev)
    obj = torch.zeros(n, dtype=torch.int32, device=dev)
    occ = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream.synchronize()
    assert d_rays.data_ptr() % 16 == 0 and d_perm_rays.data_ptr() % 16 == 0

    with lr.Context(0, tuning={"verbose": 1, "cam": 0}) as ctx:
        ctx.upload(scene)
        aov_opts = lr.render_opts(side, side, spp=1, jitter=lr.RT_JITTER_CENTER)
        launch = {
            "aov": lambda: ctx.render_aov_device(aov_opts, lr.RT_AOV_DEPTH | lr.RT_AOV_OBJECT,
                                                 {"depth": depth.data_ptr(), "object": aobj.data_ptr()}, stream.cuda_stream),
            "nearest": lambda: ctx.query_nearest_device(d_rays.data_ptr(), n, lr.RT_HIT_T | lr.RT_HIT_OBJECT,
                                                        {"t": t.data_ptr(), "object": obj.data_ptr()}, stream.cuda_stream),
            "permuted": lambda: ctx.query_nearest_device(d_perm_rays.data_ptr(), n, lr.RT_HIT_T | lr.RT_HIT_OBJECT,
                                                         {"t": t.data_ptr(), "object": obj.data_ptr()}, stream.cuda_stream),
            "occluded": lambda: ctx.query_occluded_device(d_rays.data_ptr(), 0, n, occ.data_ptr(), stream.cuda_stream),
        }

        def timed(name, k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(k):
                launch[name]()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / k

        names = ("aov", "nearest", "permuted", "occluded")
        warm = {}
        for name in ("aov", "nearest", "occluded"):
            warm[name] = timed(name, 1)
        # the query's answers on the pixels' own rays are the AOV's (the AOV's 0.0 for a miss against +inf here)
        hit = obj >= 0
        same_obj = bool(torch.equal(obj.reshape(side, side), aobj))
        same_t = bool(torch.equal(torch.where(hit, t, torch.zeros_like(t)).to(torch.float32).reshape(side, side), depth))
        same_occ = bool(torch.equal(occ != 0, hit))
        covered = float(hit.float().mean().item())
        warm["permuted"] = timed("permuted", 1)
        same_perm = bool(torch.equal(obj, aobj.reshape(-1)[perm]))
        assert same_obj and same_t and same_occ and same_perm, (same_obj, same_t, same_occ, same_perm)
        ctx.set_tuning("verbose", 0)
        launches = {k: max(1, int(args.seconds * 1e3 / args.rounds / max(warm[k], 1e-3))) for k in names}
        ms = {k: [] for k in names}
        for _ in range(args.rounds):
            for k in names:
                ms[k].append(timed(k, launches[k]))
        med = {k: statistics.median(v) for k, v in ms.items()}
    extra = n * (48 + 12 - 8)                           # what (b) moves beyond (a): 48 B in, 12 B instead of 8 B out
    moved = {"nearest": n * (48 + 12), "permuted": n * (48 + 12), "occluded": n * (48 + 1)}
    line = json.dumps({"tool": "query_bench", "scene": "config3, %d spheres" % args.spheres, "width": side, "height": side,
                       "rays": n, "device": torch.cuda.get_device_name(0), "sources_id": lr.sources_id(),
                       "rays_hit": round(covered, 4),
                       # compared before anything was timed (the run stops on a mismatch): object and f32 t of (b) against
                       # (a)'s buffers, (d)'s bytes against (b)'s hits, (c)'s objects against (a)'s permuted
                       "answers_equal_the_aov": {"object": same_obj, "t_as_f32": same_t, "occluded_is_hit": same_occ,
                                                 "permuted_object": same_perm},
                       "ms": {k: round(v, 4) for k, v in med.items()},
                       "nearest_over_aov": round(med["nearest"] / med["aov"], 3),
                       "permuted_over_nearest": round(med["permuted"] / med["nearest"], 3),
                       "occluded_over_nearest": round(med["occluded"] / med["nearest"], 3),
                       "bytes_per_ray": {"aov": {"loaded": 0, "stored": 8}, "nearest": {"loaded": 48, "stored": 12},
                                         "occluded": {"loaded": 48, "stored": 1}},
                       "nearest_extra_bytes": extra,
                       # the rays and answers a launch streams over its whole time (a lower bound on what the memory
                       # system carried: the walk's own reads are not in it)
                       "streamed_gb_per_s": {k: round(v / med[k] / 1e6, 1) for k, v in moved.items()},
                       "launches_per_round": launches, "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
