#!/usr/bin/env python3
"""What the variance-guided colour weight costs: C3 (4096^2, 1000 spheres, depth 8) accumulated
into a moments accumulator (2 samples, random jitter), resolved into a device buffer with its variance image
(rt_accum_noise) and its feature buffers, then 5 passes with the default settings (normal_squarings 5, sigma_depth
0.05, sigma_color 1.0, sigma_variance 2, variance_floor 2^-20) on the same stream, three cases:

  plain       rt_denoise_device, NORMAL | DEPTH
  color       rt_denoise_device, NORMAL | DEPTH | COLOR: the same divisions per tap as the new weight
  variance    rt_denoise_var_device, NORMAL | DEPTH, out_variance written

One warm-up per case, then the cases alternated in rounds in this one process, each a batch between two device
events; the figure per case is the median over rounds of the time per call, the rounds are kept.  No ratio is fixed in
advance.  One JSON line goes to --out.

    python tools/denoise_var_bench.py
    python tools/denoise_var_bench.py --side 1024
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
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device time per case")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_var_bench.json"))
    args = ap.parse_args()

    import torch                     # first: the process then uses torch's HIP runtime for both
    import libraytrace as lr
    from libraytrace import scenes

    side, iters = args.side, args.iterations
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    spec = scenes.config3(side, side, n=args.spheres)

    def image(channels):
        return torch.zeros((side, side, channels) if channels > 1 else (side, side), dtype=torch.float32, device=dev)

    rgb, variance = image(3), image(3)
    guides = {"normal": image(3), "depth": image(1), "albedo": image(3)}
    out_rgb, out_var = image(3), image(1)
    out_bgr = torch.zeros((side, 3 * side), dtype=torch.uint8, device=dev)
    gptr = {k: v.data_ptr() for k, v in guides.items()}

    with lr.Context(0) as ctx:
        ctx.upload(lr.Scene.deserialize(spec.to_text()))
        opts = lr.render_opts(side, side, max_depth=args.depth, spp=2, jitter=lr.RT_JITTER_RANDOM, seed=7,
                              flags=lr.RT_OUT_RGB_F32)
        with ctx.accumulator(opts, moments=True) as acc:
            acc.add(2, stream_ptr=stream.cuda_stream)
            acc.resolve_device(rgb.data_ptr(), 0, stream_ptr=stream.cuda_stream)
            acc.noise_device(1e-3, 1.0, variance.data_ptr(), None, stream.cuda_stream)
        ctx.render_aov_device(opts, lr.RT_AOV_NORMAL | lr.RT_AOV_DEPTH | lr.RT_AOV_ALBEDO, gptr, stream.cuda_stream)
        stream.synchronize()
        noisy_pixels = int((variance.sum(dim=2) > 0).sum().item())
        nd = lr.RT_DN_NORMAL | lr.RT_DN_DEPTH
        params = {"plain": lr.denoise_params(side, side, iterations=iters, flags=nd),
                  "color": lr.denoise_params(side, side, iterations=iters, flags=nd | lr.RT_DN_COLOR),
                  "variance": lr.denoise_params(side, side, iterations=iters, flags=nd)}

        def timed(case, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                for _ in range(n):
                    if case == "variance":
                        ctx.denoise_var_device(params[case], rgb.data_ptr(), variance.data_ptr(), gptr, out_rgb.data_ptr(),
                                               out_bgr.data_ptr(), out_var.data_ptr(), stream_ptr=stream.cuda_stream)
                    else:
                        ctx.denoise_device(params[case], rgb.data_ptr(), gptr, out_rgb.data_ptr(), out_bgr.data_ptr(),
                                           stream.cuda_stream)
                b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / n

        cases = ["plain", "color", "variance"]
        warm = {c: timed(c, 1) for c in cases}
        calls = {c: max(1, int(args.seconds * 1e3 / args.rounds / max(warm[c], 1e-3))) for c in cases}
        ms = {c: [] for c in cases}
        for _ in range(args.rounds):
            for c in cases:
                ms[c].append(timed(c, calls[c]))
        med = {c: statistics.median(v) for c, v in ms.items()}

    line = json.dumps({"tool": "denoise_var_bench", "scene": "config3, %d spheres" % args.spheres, "width": side, "height": side,
                       "depth": args.depth, "samples": 2, "iterations": iters, "normal_squarings": 5, "sigma_variance": 2.0,
                       "variance_floor": 2.0 ** -20, "variant": 0, "pixels_with_variance": noisy_pixels,
                       "device": torch.cuda.get_device_name(0), "sources_id": lr.sources_id(),
                       "ms": {c: round(med[c], 4) for c in cases},
                       "rounds_ms": {c: [round(x, 4) for x in ms[c]] for c in cases},
                       "variance_over_color": round(med["variance"] / med["color"], 4),
                       "variance_over_plain": round(med["variance"] / med["plain"], 4),
                       "color_over_plain": round(med["color"] / med["plain"], 4),
                       "calls_per_round": calls})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
