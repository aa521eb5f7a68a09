#!/usr/bin/env python3
"""Antialiased frames on both schedules that render them: RT_ALGO_PATH (one work-item per
pixel, or a group of lanes per pixel) against RT_ALGO_WAVEFRONT_AA (one wavefront pass per AA
sample), DESIGN.md §3.12 / §9.

config3 (1000 spheres, 2 point lights) at depth 8 with random jitter, rt_render_device into
device buffers on one stream.  Per case: one warm-up frame per schedule (compared bit for bit,
f32 and BGR, at the timed size), then the two schedules alternated in rounds in this one
process, each round timing a batch of frames between two device events, until each schedule
has run for about --seconds.  The figure per schedule is the median over rounds of the
batch's time per frame.  One JSON line goes to --out (under profiles/).

    python tools/aa_bench.py                     # 2048^2 and 4096^2 at spp 4 and 16, 256^2 at spp 256
    python tools/aa_bench.py --cases 256x256     # side x spp, comma separated
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
    ap.add_argument("--cases", default="2048x4,2048x16,4096x4,4096x16,256x256")
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device time per schedule and case")
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the two schedules per case")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aa_bench.json"))
    args = ap.parse_args()

    import torch                     # first: the process then uses torch's HIP runtime for both
    import libraytrace as lr
    from libraytrace import scenes

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    algos = (("path", lr.RT_ALGO_PATH), ("wavefront_aa", lr.RT_ALGO_WAVEFRONT_AA))
    results = []
    with lr.Context(0) as ctx:
        for case in args.cases.split(","):
            side, spp = (int(x) for x in case.split("x"))
            spec = scenes.config3(side, side)
            ctx.upload(lr.Scene.deserialize(spec.to_text()))
            outs = {}

            def frame(name, algo):
                o = lr.render_opts(side, side, max_depth=args.depth, spp=spp, algo=algo, jitter=lr.RT_JITTER_RANDOM,
                                   seed=args.seed)
                rgb, bgr = outs[name]
                ctx.render_device(o, rgb.data_ptr(), bgr.data_ptr(), stream.cuda_stream)

            def timed(name, algo, n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(n):
                    frame(name, algo)
                b.record(stream)
                b.synchronize()
                return a.elapsed_time(b) / n

            warm = {}
            for name, algo in algos:
                outs[name] = (torch.zeros((side, side, 3), dtype=torch.float32, device=dev),
                              torch.zeros((side, 3 * side), dtype=torch.uint8, device=dev))
                ctx.reserve(lr.render_opts(side, side, max_depth=args.depth, spp=spp, algo=algo,
                                           jitter=lr.RT_JITTER_RANDOM, seed=args.seed), stream_ptr=stream.cuda_stream)
                warm[name] = timed(name, algo, 1)
            st = ctx.stats()
            equal = bool(torch.equal(outs["path"][0].view(torch.int32), outs["wavefront_aa"][0].view(torch.int32)) and
                         torch.equal(outs["path"][1], outs["wavefront_aa"][1]))
            ms = {name: [] for name, _ in algos}
            frames = {name: max(1, int(args.seconds * 1e3 / args.rounds / max(warm[name], 1e-3))) for name, _ in algos}
            for _ in range(args.rounds):
                for name, algo in algos:
                    ms[name].append(timed(name, algo, frames[name]))
            med = {name: statistics.median(v) for name, v in ms.items()}
            results.append({"width": side, "height": side, "spp": spp, "depth": args.depth, "rays_per_frame": int(st.rays),
                            "bit_equal": equal,
                            "path_ms": round(med["path"], 4), "wavefront_aa_ms": round(med["wavefront_aa"], 4),
                            "path_over_wavefront_aa": round(med["path"] / med["wavefront_aa"], 3),
                            "frames_per_round": frames, "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}})
            print(json.dumps(results[-1]), file=sys.stderr, flush=True)
            del outs
    line = json.dumps({"tool": "aa_bench", "scene": "config3", "jitter": "random", "seed": args.seed,
                       "device": torch.cuda.get_device_name(0), "sources_id": lr.sources_id(), "cases": results})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if all(r["bit_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
