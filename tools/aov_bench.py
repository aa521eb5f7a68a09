#!/usr/bin/env python3
"""First-hit feature buffers against the camera pass they share their walk with:
C3 (4096^2, 1000 spheres) at spp 1 with centre jitter, rt_render_aov_device into device buffers on one stream.

  (a) aov_all     every channel: depth, normal, albedo, coverage, object (36 B of stores per pixel)
  (b) aov_depth   the depth channel alone (4 B per pixel)
  (c) camera      the camera pass (RT_KF_CAMERA) of the ordinary RT_ALGO_WAVEFRONT frame at depth 8, from the
                  per-launch events of RT_TIME_KERNELS frames (rt_ctx_kernel_times)
One warm-up per case, then the cases alternated in rounds in this one process: (a) and (b) time a batch of
renders between two device events, (c) sums the camera launches of a batch of timed frames, until each case has
run for about --seconds.  The figure per case is the median over rounds of the time per render; the rounds are
kept.  The camera pass is the yardstick, not a gate: aov_primary does its walk, plus a normal, plus the stores.
One JSON line goes to --out (under profiles/).  No step is tried twice.

    python tools/aov_bench.py
    python tools/aov_bench.py --side 1024
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rust-raytrace_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--spheres", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device time per case")
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the cases")
    ap.add_argument("--depth", type=int, default=8, help="max_depth of the wavefront frames whose camera pass is timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aov_bench.json"))
    args = ap.parse_args()

    import torch                     # first: the process then uses torch's HIP runtime for both
    import libraytrace as lr
    from libraytrace import scenes

    side = args.side
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    spec = scenes.config3(side, side, n=args.spheres)
    bufs = {"depth": torch.zeros((side, side), dtype=torch.float32, device=dev),
            "normal": torch.zeros((side, side, 3), dtype=torch.float32, device=dev),
            "albedo": torch.zeros((side, side, 3), dtype=torch.float32, device=dev),
            "coverage": torch.zeros((side, side), dtype=torch.float32, device=dev),
            "object": torch.zeros((side, side), dtype=torch.int32, device=dev)}
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    rgb = torch.zeros((side, side, 3), dtype=torch.float32, device=dev)
    bgr = torch.zeros((side, 3 * side), dtype=torch.uint8, device=dev)
    masks = {"aov_all": lr.RT_AOV_ALL, "aov_depth": lr.RT_AOV_DEPTH}

    with lr.Context(0, tuning={"verbose": 1}) as ctx:
        ctx.upload(lr.Scene.deserialize(spec.to_text()))
        aov_opts = lr.render_opts(side, side, spp=1, jitter=lr.RT_JITTER_CENTER)
        wf_opts = lr.render_opts(side, side, max_depth=args.depth, spp=1, jitter=lr.RT_JITTER_CENTER,
                                 algo=lr.RT_ALGO_WAVEFRONT,
                                 flags=lr.RT_OUT_RGB_F32 | lr.RT_OUT_BGR_U8 | lr.RT_TIME_KERNELS)
        ctx.reserve(wf_opts, stream_ptr=stream.cuda_stream)

        def timed(name, n):
            if name == "camera":
                ctx.kernel_times()
                for _ in range(n):
                    ctx.render_device(wf_opts, rgb.data_ptr(), bgr.data_ptr(), stream.cuda_stream)
                stream.synchronize()             # every stream of the frames has joined: all their events are complete
                ms, launches = ctx.kernel_times()["camera"]
                assert launches == n, (launches, n)
                return ms / n
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(n):
                ctx.render_aov_device(aov_opts, masks[name], ptrs, stream.cuda_stream)
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / n

        names = ("aov_all", "aov_depth", "camera")
        warm = {n: timed(n, 1) for n in names}
        ctx.set_tuning("verbose", 0)
        st = ctx.stats()
        covered = float((bufs["coverage"] > 0).float().mean().item())
        frames = {n: max(1, int(args.seconds * 1e3 / args.rounds / max(warm[n], 1e-3))) for n in names}
        # (a batch of timed frames records two events per launch: within the context's event pool)
        frames["camera"] = min(frames["camera"], 200)
        ms = {n: [] for n in names}
        for _ in range(args.rounds):
            for n in names:
                ms[n].append(timed(n, frames[n]))
        med = {k: statistics.median(v) for k, v in ms.items()}
    line = json.dumps({"tool": "aov_bench", "scene": "config3, %d spheres" % args.spheres, "width": side, "height": side,
                       "spp": 1, "jitter": "centre", "wavefront_depth": args.depth,
                       "device": torch.cuda.get_device_name(0), "sources_id": lr.sources_id(),
                       "pixels_hit": round(covered, 4), "camera_pass_rays": int(st.pixels),
                       "ms": {k: round(v, 4) for k, v in med.items()},
                       "aov_all_over_camera": round(med["aov_all"] / med["camera"], 3),
                       "aov_depth_over_camera": round(med["aov_depth"] / med["camera"], 3),
                       "bytes_stored_per_pixel": {"aov_all": 36, "aov_depth": 4},
                       "frames_per_round": frames, "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
