"""A/B of one denoising step with FreeU off and on at the metric configuration (fp16, 16 frames of 64x64 latents, guidance batch 2,
hipGraph replay): two instances of the same seeded v1.02 UNet, one with `enable_freeu`, their replayed forwards timed alternately in
one process with device events; then the six aa_freeu_tokens launches of a step timed one by one inside eager forwards.

    python scripts/bench_freeu.py [--steps 20] [--warmup 5] [--out profiles/freeu_ab.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FREEU = dict(s1=0.9, s2=0.2, b1=1.2, b2=1.4)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--lat", type=int, default=64)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert a.steps >= 20 and a.warmup >= 5, "at least 5 warm-up and 20 timed steps"
    import bench
    from animate_anything_amd import ops
    from util import fullsize_inputs
    dev = torch.device("cuda:0")
    off = bench.build_unet(torch.float16, dev)
    on = copy.deepcopy(off)
    on.enable_freeu(**FREEU)
    i = fullsize_inputs(a.frames, a.lat)
    h = lambda x: x.half().to(dev)
    args = (h(i["sample"]), i["t"], h(i["text"]), h(i["cond"]), h(i["mask"]))

    def step(net):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        net(*args, motion=i["motion"])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {"off": [], "on": []}
    with torch.no_grad():
        for net in (off, on):
            net.enable_graph()
        for k in range(a.warmup + a.steps):                      # alternately, so drift of the clocks hits both alike
            for name, net in (("off", off), ("on", on)):
                ms = step(net)
                if k >= a.warmup:
                    times[name].append(ms)
        # the six launches, each between its own pair of events, inside eager forwards of the FreeU model
        on.enable_graph(False)
        real, pairs = ops.freeu, []

        def timed_freeu(*x, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = real(*x, **k)
            e1.record()
            pairs.append(((x[2], x[3], x[4], x[0].shape[1], x[1].shape[1]), e0, e1))
            return out

        ops.freeu = timed_freeu
        launches = {}
        try:
            for k in range(a.warmup + a.steps):
                del pairs[:]
                on(*args, motion=i["motion"])
                torch.cuda.synchronize()
                assert len(pairs) == 6
                if k >= a.warmup:
                    for n, (shape, e0, e1) in enumerate(pairs):
                        launches.setdefault((n, shape), []).append(e0.elapsed_time(e1))
        finally:
            ops.freeu = real
    off_med, on_med = statistics.median(times["off"]), statistics.median(times["on"])
    per_launch = [dict(launch=n, images=s[0], h=s[1], w=s[2], c_hidden=s[3], c_skip=s[4],
                       mbytes_moved=round(s[0] * s[1] * s[2] * (s[3] + 2 * s[4]) * 2 / 1e6, 1), **stats(ms))
                  for (n, s), ms in sorted(launches.items())]
    result = {"what": "UNet3D forward of one guided denoising step (graph replay), FreeU off / on, timed alternately",
              "device": torch.cuda.get_device_name(0), "frames": a.frames, "latents": a.lat, "dtype": "fp16", "freeu": FREEU,
              "step_off": stats(times["off"]), "step_on": stats(times["on"]),
              "on_minus_off_ms": round(on_med - off_med, 4), "on_minus_off_percent_of_step": round(100 * (on_med - off_med) / off_med, 3),
              "freeu_launches_eager": per_launch,
              "freeu_launches_sum_of_medians_ms": round(sum(x["median_ms"] for x in per_launch), 4),
              "note": "mbytes_moved: hidden half read + written in place (c_hidden / 2 columns each way), skip read once (planes up to "
                      "256 pixels stay in registers) and written once"}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
