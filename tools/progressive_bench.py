#!/usr/bin/env python3
"""What progressive rendering costs: a frame rendered as steps of K samples (rt_render_accumulate)
with one resolve per step (rt_accum_resolve), against the one-shot rt_render_device of the same
frame, DESIGN.md §3.14.

config3 (1000 spheres, 2 point lights) at depth 8 with random jitter, device buffers, one stream,
on RT_ALGO_PATH and RT_ALGO_WAVEFRONT_AA.  Per case (side x spp) and algorithm: the one-shot frame
and the frame in steps of K in {1, 4, 16, all} are warmed up once (and compared bit for bit, f32 and
BGR), then alternated in rounds in this one process, each round timing a batch of frames between
two device events, until each variant has run for about --seconds.  The figure per variant is the
median over rounds of the batch's time per frame; `over_one_shot` is its ratio to the one-shot
frame's.  One resolve alone (the kernel's cost per step) is timed the same way.  One JSON line
goes to --out (under profiles/).

    python tools/progressive_bench.py                      # 256^2 x 64 and 1024^2 x 16
    python tools/progressive_bench.py --cases 256x64       # side x spp, comma separated
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
    ap.add_argument("--steps", default="1,4,16,all")
    ap.add_argument("--seconds", type=float, default=0.6, help="timed device time per variant")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the variants per case and algorithm")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progressive_bench.json"))
    args = ap.parse_args()

    import torch                     # first: the process then uses torch's HIP runtime for both
    import libraytrace as lr
    from libraytrace import scenes

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    algos = (("path", lr.RT_ALGO_PATH), ("wavefront_aa", lr.RT_ALGO_WAVEFRONT_AA))
    results = []
    with lr.Context(0) as ctx:
        for case in args.cases.split(","):
            side, spp = (int(x) for x in case.split("x"))
            spec = scenes.config3(side, side)
            ctx.upload(lr.Scene.deserialize(spec.to_text()))
            steps = sorted({spp if s == "all" else min(int(s), spp) for s in args.steps.split(",")})
            for name, algo in algos:
                o = lr.render_opts(side, side, max_depth=args.depth, spp=spp, algo=algo, jitter=lr.RT_JITTER_RANDOM,
                                   seed=args.seed)
                one = (torch.zeros((side, side, 3), dtype=torch.float32, device=dev),
                       torch.zeros((side, 3 * side), dtype=torch.uint8, device=dev))
                out = (torch.zeros_like(one[0]), torch.zeros_like(one[1]))
                ctx.reserve(o, stream_ptr=sp)
                acc = ctx.accumulator(o)

                def one_shot():
                    ctx.render_device(o, one[0].data_ptr(), one[1].data_ptr(), sp)

                def in_steps(k):
                    def frame():
                        acc.reset()
                        done = 0
                        while done < spp:
                            n = min(k, spp - done)
                            acc.add(n, algo, stream_ptr=sp)
                            acc.resolve_device(out[0].data_ptr(), out[1].data_ptr(), stream_ptr=sp)
                            done += n
                    return frame

                def resolve_only():
                    acc.resolve_device(out[0].data_ptr(), out[1].data_ptr(), stream_ptr=sp)

                def timed(fn, n):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    for _ in range(n):
                        fn()
                    b.record(stream)
                    b.synchronize()
                    return a.elapsed_time(b) / n

                variants = [("one_shot", one_shot)] + [(f"steps_of_{k}", in_steps(k)) for k in steps]
                warm, equal = {}, {}
                for vname, fn in variants:
                    warm[vname] = timed(fn, 1)
                    if vname != "one_shot":
                        equal[vname] = bool(torch.equal(one[0].view(torch.int32), out[0].view(torch.int32)) and
                                            torch.equal(one[1], out[1]))
                variants.append(("resolve", resolve_only))
                warm["resolve"] = timed(resolve_only, 4)
                ms = {v: [] for v, _ in variants}
                frames = {v: max(1, int(args.seconds * 1e3 / args.rounds / max(warm[v], 1e-3))) for v, _ in variants}
                for _ in range(args.rounds):
                    for vname, fn in variants:
                        ms[vname].append(timed(fn, frames[vname]))
                med = {v: statistics.median(x) for v, x in ms.items()}
                acc.close()
                results.append({"width": side, "height": side, "spp": spp, "depth": args.depth, "algo": name,
                                "bit_equal": equal, "ms": {v: round(x, 4) for v, x in med.items()},
                                "over_one_shot": {v: round(med[v] / med["one_shot"], 3) for v in med
                                                  if v.startswith("steps_of_")},
                                "steps_per_frame": {f"steps_of_{k}": -(-spp // k) for k in steps},
                                "frames_per_round": frames,
                                "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}})
                print(json.dumps(results[-1]), file=sys.stderr, flush=True)
                del one, out
    line = json.dumps({"tool": "progressive_bench", "scene": "config3", "jitter": "random", "seed": args.seed,
                       "device": torch.cuda.get_device_name(0), "sources_id": lr.sources_id(), "cases": results})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if all(all(r["bit_equal"].values()) for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
