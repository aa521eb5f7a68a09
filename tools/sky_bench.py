#!/usr/bin/env python3
"""Skybox frames on the schedules that render them: a 1000-sphere mirror
scene (random_spheres' config3 plus six 512x512 faces; every fifth sphere a mirror) at depth 8.

Per size, rt_render_device into device buffers on one stream:
  (a) path            RT_ALGO_PATH, centre jitter         (how the scene rendered before)
  (b) wavefront       RT_ALGO_WAVEFRONT, centre jitter
  (c) wavefront_solid RT_ALGO_WAVEFRONT, the same scene with a solid background (what the sky costs)
  (d) path_aa / wavefront_aa   spp 4, random jitter: RT_ALGO_PATH against RT_ALGO_WAVEFRONT_AA
One warm-up frame per case (the sky cases compared bit for bit, f32 and BGR, within (a, b) and
within (d)), then the cases alternated in rounds in this one process, each round timing a batch of
frames between two device events, until each case has run for about --seconds.  The figure per
case is the median over rounds of the batch's time per frame; the rounds are kept.  One JSON line
goes to --out (under profiles/).  No step is tried twice.

    python tools/sky_bench.py                       # 1024^2, 2048^2, 4096^2
    python tools/sky_bench.py --sides 1024
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rust-raytrace_amd")]


def mirror_scene(scenes, side, paths):
    spec = scenes.config3(side, side)
    for o in spec.objects[::5]:
        o["material"] = scenes.phong((0.05, 0.05, 0.05), (0.9, 0.9, 0.9), 64.0, (0.0, 0.0, 0.0))
    spec.skybox = list(paths) if paths else None
    return spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="1024,2048,4096")
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device time per case and size")
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the cases per size")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--face", type=int, default=512)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky_bench.json"))
    args = ap.parse_args()

    import torch                     # first: the process then uses torch's HIP runtime for both
    import numpy as np
    import libraytrace as lr
    from libraytrace import scenes

    tmp = tempfile.mkdtemp(prefix="sky_bench_")
    paths = [os.path.join(tmp, f"f{k}.ppm") for k in range(6)]
    rng = np.random.default_rng(args.seed)
    yy, xx = np.mgrid[0:args.face, 0:args.face]
    for k, p in enumerate(paths):            # gradients + noise, a tint per face (skybox_faces, vectorised)
        base = np.stack([40 + 30 * k + (6 * xx) % 160, 200 - (8 * yy) % 190, 90 + 20 * ((xx + yy + k) % 5)], axis=-1)
        scenes.write_ppm(p, np.clip(base + rng.integers(0, 23, base.shape), 0, 255).astype(np.uint8))

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    C, R = lr.RT_JITTER_CENTER, lr.RT_JITTER_RANDOM
    cases = (("path", True, lr.RT_ALGO_PATH, C, 1), ("wavefront", True, lr.RT_ALGO_WAVEFRONT, C, 1),
             ("wavefront_solid", False, lr.RT_ALGO_WAVEFRONT, C, 1),
             ("path_aa", True, lr.RT_ALGO_PATH, R, 4), ("wavefront_aa", True, lr.RT_ALGO_WAVEFRONT_AA, R, 4))
    results = []
    with lr.Context(0) as sky_ctx, lr.Context(0) as solid_ctx:
        for side in (int(s) for s in args.sides.split(",")):
            sky_ctx.upload(lr.Scene.deserialize(mirror_scene(scenes, side, paths).to_text()))
            solid_ctx.upload(lr.Scene.deserialize(mirror_scene(scenes, side, None).to_text()))
            outs = {}

            def opts(algo, jitter, spp):
                return lr.render_opts(side, side, max_depth=args.depth, spp=spp, algo=algo, jitter=jitter, seed=args.seed)

            def timed(case, n):
                name, sky, algo, jitter, spp = case
                ctx = sky_ctx if sky else solid_ctx
                rgb, bgr = outs[name]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(n):
                    ctx.render_device(opts(algo, jitter, spp), rgb.data_ptr(), bgr.data_ptr(), stream.cuda_stream)
                b.record(stream)
                b.synchronize()
                return a.elapsed_time(b) / n

            warm, rays = {}, {}
            for case in cases:
                name, sky, algo, jitter, spp = case
                outs[name] = (torch.zeros((side, side, 3), dtype=torch.float32, device=dev),
                              torch.zeros((side, 3 * side), dtype=torch.uint8, device=dev))
                (sky_ctx if sky else solid_ctx).reserve(opts(algo, jitter, spp), stream_ptr=stream.cuda_stream)
                warm[name] = timed(case, 1)
                rays[name] = int((sky_ctx if sky else solid_ctx).stats().rays)

            def same(a, b):
                return bool(torch.equal(outs[a][0].view(torch.int32), outs[b][0].view(torch.int32)) and
                            torch.equal(outs[a][1], outs[b][1]))

            equal = {"wavefront_vs_path": same("path", "wavefront"), "wavefront_aa_vs_path": same("path_aa", "wavefront_aa")}
            ms = {c[0]: [] for c in cases}
            frames = {c[0]: max(1, int(args.seconds * 1e3 / args.rounds / max(warm[c[0]], 1e-3))) for c in cases}
            for _ in range(args.rounds):
                for case in cases:
                    ms[case[0]].append(timed(case, frames[case[0]]))
            med = {k: statistics.median(v) for k, v in ms.items()}
            results.append({"width": side, "height": side, "depth": args.depth, "rays_per_frame": rays, "bit_equal": equal,
                            "ms": {k: round(v, 4) for k, v in med.items()},
                            "path_over_wavefront": round(med["path"] / med["wavefront"], 3),
                            "sky_over_solid": round(med["wavefront"] / med["wavefront_solid"], 3),
                            "path_aa_over_wavefront_aa": round(med["path_aa"] / med["wavefront_aa"], 3),
                            "frames_per_round": frames, "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}})
            print(json.dumps(results[-1]), file=sys.stderr, flush=True)
            del outs
    line = json.dumps({"tool": "sky_bench", "scene": "config3, every fifth sphere a mirror, six %d^2 faces" % args.face,
                       "seed": args.seed, "device": torch.cuda.get_device_name(0), "sources_id": lr.sources_id(),
                       "cases": results})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if all(all(r["bit_equal"].values()) for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
