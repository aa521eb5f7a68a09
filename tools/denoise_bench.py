#!/usr/bin/env python3
"""The denoiser against the traffic it cannot avoid and against the frame it follows: C3
(4096^2, 1000 spheres, depth 8) rendered into device buffers with its feature buffers, then rt_denoise_device with
the default settings (NORMAL | DEPTH, normal_squarings 5, sigma_depth 0.05) on the same stream.

  per variant (1 direct, 2 LDS tiles at steps 1 and 2) and per iteration count n = 1 .. --iterations:
      total(n)    one call of n passes (pack pass + n - 1 inner passes + the last pass)
      added(n)    total(n) - total(n - 1): what pass n - 1 (step 2^(n-1)) adds as an inner pass
  copy        a device-to-device copy of 24 B per pixel (48 B per pixel of traffic: what an inner pass must move at the
              least, a colour and a guide record read and a colour record written, 16 B each), the yardstick
  frame       the C3 frame (rt_render_device, RT_ALGO_AUTO) of the same run
One warm-up per case, then the cases alternated in rounds in this one process, each a batch between two device
events; the figure per case is the median over rounds of the time per call, the rounds are kept.  No threshold:
the faster variant is the default (render_plan.hpp, kDnAutoVariant).  One JSON line goes to --out.

    python tools/denoise_bench.py
    python tools/denoise_bench.py --side 1024
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
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed device time per case")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.json"))
    args = ap.parse_args()

    import torch                     # first: the process then uses torch's HIP runtime for both
    import libraytrace as lr
    from libraytrace import scenes

    side, iters = args.side, args.iterations
    npix = side * side
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    spec = scenes.config3(side, side, n=args.spheres)
    rgb = torch.zeros((side, side, 3), dtype=torch.float32, device=dev)
    guides = {"normal": torch.zeros((side, side, 3), dtype=torch.float32, device=dev),
              "depth": torch.zeros((side, side), dtype=torch.float32, device=dev),
              "albedo": torch.zeros((side, side, 3), dtype=torch.float32, device=dev)}
    out_rgb = torch.zeros((side, side, 3), dtype=torch.float32, device=dev)
    out_bgr = torch.zeros((side, 3 * side), dtype=torch.uint8, device=dev)
    copy_src = torch.zeros(npix * 24, dtype=torch.uint8, device=dev)
    copy_dst = torch.zeros(npix * 24, dtype=torch.uint8, device=dev)
    gptr = {k: v.data_ptr() for k, v in guides.items()}

    with lr.Context(0) as ctx:
        ctx.upload(lr.Scene.deserialize(spec.to_text()))
        frame_opts = lr.render_opts(side, side, max_depth=args.depth, spp=1, jitter=lr.RT_JITTER_CENTER,
                                    flags=lr.RT_OUT_RGB_F32)
        ctx.reserve(frame_opts, stream_ptr=stream.cuda_stream)
        ctx.render_device(frame_opts, rgb.data_ptr(), 0, stream.cuda_stream)
        ctx.render_aov_device(frame_opts, lr.RT_AOV_NORMAL | lr.RT_AOV_DEPTH | lr.RT_AOV_ALBEDO, gptr, stream.cuda_stream)
        stream.synchronize()
        params = {(v, n): lr.denoise_params(side, side, iterations=n, variant=v) for v in (1, 2) for n in range(1, iters + 1)}

        def timed(case, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                for _ in range(n):
                    if case == "copy":
                        copy_dst.copy_(copy_src, non_blocking=True)
                    elif case == "frame":
                        ctx.render_device(frame_opts, rgb.data_ptr(), 0, stream.cuda_stream)
                    else:
                        ctx.denoise_device(params[case], rgb.data_ptr(), gptr, out_rgb.data_ptr(), out_bgr.data_ptr(),
                                           stream.cuda_stream)
                b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / n

        cases = ["copy", "frame"] + sorted(params)
        warm = {c: timed(c, 1) for c in cases}
        calls = {c: max(1, int(args.seconds * 1e3 / args.rounds / max(warm[c], 1e-3))) for c in cases}
        ms = {c: [] for c in cases}
        for _ in range(args.rounds):
            for c in cases:
                ms[c].append(timed(c, calls[c]))
        med = {c: statistics.median(v) for c, v in ms.items()}

    def variant(v):
        total = [med[(v, n)] for n in range(1, iters + 1)]
        return {"total_ms": [round(x, 4) for x in total],
                "added_ms": [round(total[i] - total[i - 1], 4) for i in range(1, iters)],
                "rounds_ms": {str(n): [round(x, 4) for x in ms[(v, n)]] for n in range(1, iters + 1)}}

    traffic = 48 * npix
    direct, lds = variant(1), variant(2)
    faster = 1 if direct["total_ms"][-1] <= lds["total_ms"][-1] else 2
    best = min(direct["total_ms"][-1], lds["total_ms"][-1])
    line = json.dumps({"tool": "denoise_bench", "scene": "config3, %d spheres" % args.spheres, "width": side, "height": side,
                       "depth": args.depth, "iterations": iters, "flags": "NORMAL|DEPTH", "normal_squarings": 5,
                       "device": torch.cuda.get_device_name(0), "sources_id": lr.sources_id(),
                       "direct": direct, "lds": lds, "faster_variant": faster,
                       "inner_pass_min_bytes": traffic, "last_pass_min_bytes": (32 + 15) * npix,
                       "copy_ms": round(med["copy"], 4), "copy_GBps": round(traffic / med["copy"] / 1e6, 1),
                       "inner_pass_GBps": {"direct": [round(traffic / x / 1e6, 1) if x > 0 else None for x in direct["added_ms"]],
                                           "lds": [round(traffic / x / 1e6, 1) if x > 0 else None for x in lds["added_ms"]]},
                       "frame_ms": round(med["frame"], 4), "denoise_over_frame": round(best / med["frame"], 3),
                       "calls_per_round": {str(k): v for k, v in calls.items()},
                       "rounds_ms": {"copy": [round(x, 4) for x in ms["copy"]], "frame": [round(x, 4) for x in ms["frame"]]}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
