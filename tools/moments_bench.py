#!/usr/bin/env python3
"""What second moments cost: a frame accumulated in steps of K samples on a plain accumulator, on a
moments accumulator (rt_accum_create_moments), and on a moments accumulator with one rt_accum_noise
after every step, DESIGN.md §3.19.

tools/progressive_bench.py's frames: config3 (1000 spheres, 2 point lights) at depth 8 with random
jitter, 256^2 x 64 and 1024^2 x 16, on RT_ALGO_PATH and RT_ALGO_WAVEFRONT_AA, K in {4, 16}, one
stream.  Per case, algorithm and K the three variants are warmed up once (the moments accumulator's
sums compared bit for bit with the plain one's), then alternated in rounds in this one process, each
round timing a batch of frames between two device events; the figure per variant is the median over
rounds of the batch's time per frame, `over_plain` its ratio to the plain accumulator's.  rt_accum_noise
returns its count, so the third variant synchronises with the device once per step; the others do not.
accum_noise alone (variance and error written) is timed the same way against a device-to-device copy
of the traffic it must move, 48 B in and 16 B out per pixel: a copy of 32 B per pixel reads and writes
64 B per pixel in all.  One JSON line goes to --out (under profiles/).

    python tools/moments_bench.py                      # 256^2 x 64 and 1024^2 x 16
    python tools/moments_bench.py --cases 256x64       # side x spp, comma separated
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
    ap.add_argument("--cases", default="256x64,1024x16")
    ap.add_argument("--steps", default="4,16")
    ap.add_argument("--seconds", type=float, default=0.6, help="timed device time per variant")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the variants per case, algorithm and K")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch                     # first: the process then uses torch's HIP runtime for both
    import libraytrace as lr
    from libraytrace import scenes

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    algos = (("path", lr.RT_ALGO_PATH), ("wavefront_aa", lr.RT_ALGO_WAVEFRONT_AA))
    results = []

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(n):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / n

    with lr.Context(0) as ctx:
        for case in args.cases.split(","):
            side, spp = (int(x) for x in case.split("x"))
            spec = scenes.config3(side, side)
            ctx.upload(lr.Scene.deserialize(spec.to_text()))
            var = torch.zeros((side, side, 3), dtype=torch.float32, device=dev)
            err = torch.zeros((side, side), dtype=torch.float32, device=dev)
            src = torch.zeros(side * side * 32, dtype=torch.uint8, device=dev)
            dst = torch.zeros_like(src)
            for name, algo in algos:
                o = lr.render_opts(side, side, max_depth=args.depth, spp=spp, algo=algo, jitter=lr.RT_JITTER_RANDOM,
                                   seed=args.seed)
                ctx.reserve(o, stream_ptr=sp)
                plain, mom = ctx.accumulator(o), ctx.accumulator(o, moments=True)
                above = {}

                def in_steps(acc, k, noise):
                    def frame():
                        acc.reset()
                        done = 0
                        while done < spp:
                            n = min(k, spp - done)
                            acc.add(n, algo, stream_ptr=sp)
                            done += n
                            if noise and done >= 2:
                                above[k] = acc.noise_device(args.floor, args.threshold, var.data_ptr(), err.data_ptr(), sp)
                    return frame

                def noise_only():
                    mom.noise_device(args.floor, args.threshold, var.data_ptr(), err.data_ptr(), sp)

                def copy_only():
                    with torch.cuda.stream(stream):
                        dst.copy_(src)

                for k in sorted({min(int(s), spp) for s in args.steps.split(",")}):
                    variants = [("plain", in_steps(plain, k, False)), ("moments", in_steps(mom, k, False)),
                                ("moments_noise", in_steps(mom, k, True))]
                    warm = {v: timed(fn, 1) for v, fn in variants}
                    equal = bool(np.array_equal(plain.download()[0].view(np.uint64), mom.download()[0].view(np.uint64)))
                    variants += [("noise", noise_only), ("copy_32B_per_pixel", copy_only)]
                    warm["noise"], warm["copy_32B_per_pixel"] = timed(noise_only, 4), timed(copy_only, 4)
                    ms = {v: [] for v, _ in variants}
                    frames = {v: max(1, int(args.seconds * 1e3 / args.rounds / max(warm[v], 1e-3))) for v, _ in variants}
                    for _ in range(args.rounds):
                        for vname, fn in variants:
                            ms[vname].append(timed(fn, frames[vname]))
                    med = {v: statistics.median(x) for v, x in ms.items()}
                    results.append({"width": side, "height": side, "spp": spp, "depth": args.depth, "algo": name, "K": k,
                                    "sums_bit_equal": equal, "above_at_end": above.get(k),
                                    "ms": {v: round(x, 4) for v, x in med.items()},
                                    "over_plain": {v: round(med[v] / med["plain"], 3) for v in ("moments", "moments_noise")},
                                    "noise_over_copy": round(med["noise"] / med["copy_32B_per_pixel"], 3),
                                    "steps_per_frame": -(-spp // k), "frames_per_round": frames,
                                    "rounds_ms": {v: [round(x, 4) for x in xs] for v, xs in ms.items()}})
                    print(json.dumps(results[-1]), file=sys.stderr, flush=True)
                plain.close()
                mom.close()
            del var, err, src, dst
    line = json.dumps({"tool": "moments_bench", "scene": "config3", "jitter": "random", "seed": args.seed,
                       "floor": args.floor, "threshold": args.threshold, "device": torch.cuda.get_device_name(0),
                       "sources_id": lr.sources_id(), "cases": results})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if all(r["sums_bit_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
