"""What a context-window step costs at the metric configuration (fp16, 64x64 latents, guidance 9, hipGraph replay, DPM-Solver++): one
seeded v1.02 UNet in one process, `LatentToVideoPipeline.denoise` run alternately on
  * 16 frames without windows - the plain fused step: session replay + solver kernel - and
  * 32 frames with `context=dict(frames=16, overlap=4)` - three windows per step, each aa_window_gather_latents + the SAME 16-frame
    session replay + aa_window_merge_tokens, then one solver kernel over 32 frames,
a device event recorded in the per-step callback: the time between two callbacks is one step.  Reported: the windowed step, three times
the plain step, and the difference per window (what gather + merge + the longer solver kernel add to a replay).  Then the gather and the
merge alone, between their own pairs of events.

    python scripts/bench_context_windows.py [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/context_windows_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GUIDANCE = 9.0
CONTEXT = dict(frames=16, overlap=4, weights="pyramid")


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20, help="timed steps per variant, spread over the rounds")
    p.add_argument("--warmup", type=int, default=5, help="untimed steps in front of every run")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--frames", type=int, default=32, help="frames of the windowed clip")
    p.add_argument("--lat", type=int, default=64)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert a.steps >= 20 and a.warmup >= 5, "at least 5 warm-up and 20 timed steps"
    import bench
    from animate_anything_amd import ops
    from animate_anything_amd.pipeline import LatentToVideoPipeline
    from animate_anything_amd.schedulers import DPMSolverMultistepScheduler, context_windows
    dev = torch.device("cuda:0")
    unet = bench.build_unet(torch.float16, dev)
    unet.enable_graph()
    pipe = LatentToVideoPipeline(vae=None, unet=unet, scheduler=DPMSolverMultistepScheduler())
    short = bench.synthetic_inputs(CONTEXT["frames"], a.lat, torch.float16, dev)
    long_latents = torch.randn(1, 4, a.frames, a.lat, a.lat, generator=torch.Generator().manual_seed(5)).to(dev)
    embeds = torch.cat([short["neg"], short["text"]])
    windows = len(context_windows(a.frames, CONTEXT["frames"], CONTEXT["overlap"]))
    per_round = -(-a.steps // a.rounds)
    pipe.scheduler.set_timesteps(a.warmup + per_round + 1)
    ts = [int(t) for t in pipe.scheduler.timesteps][:a.warmup + per_round + 1]

    def run(windowed):
        """One denoise call; returns the milliseconds between consecutive callbacks behind the warm-up."""
        marks = []

        def mark(i, t, x):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append(e)
        latents = long_latents.clone() if windowed else short["latents"].clone()
        pipe.denoise(latents, embeds, short["cond"], short["mask"], [3.0], ts, GUIDANCE, callback=mark, context=CONTEXT if windowed else None)
        torch.cuda.synchronize()
        return [marks[k].elapsed_time(marks[k + 1]) for k in range(a.warmup, len(marks) - 1)]

    times = {"plain": [], "windowed": []}
    with torch.no_grad():
        run(False), run(True)                                     # capture, tile choices
        for _ in range(a.rounds):                                 # alternately, so drift of the clocks hits both alike
            times["plain"] += run(False)
            times["windowed"] += run(True)
        # the two window launches alone, between their own events
        pairs = {"window_gather_latents": [], "window_merge_tokens": []}
        real = {name: getattr(ops, name) for name in pairs}

        def timed(name):
            def call(*x, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = real[name](*x, **k)
                e1.record()
                pairs[name].append((e0, e1))
                return out
            return call
        for name in pairs:
            setattr(ops, name, timed(name))
        try:
            run(True)
        finally:
            for name in pairs:
                setattr(ops, name, real[name])
        launches = {name: [e0.elapsed_time(e1) for e0, e1 in v[a.warmup * windows:]] for name, v in pairs.items()}
    plain, windowed = statistics.median(times["plain"]), statistics.median(times["windowed"])
    hw = a.lat * a.lat
    result = {"what": "one guided denoising step: 16 frames plain (graph replay + solver kernel) against %d frames in %d windows of 16 "
                      "(per window gather + the same replay + merge, then one solver kernel), runs alternated" % (a.frames, windows),
              "device": torch.cuda.get_device_name(0), "frames": a.frames, "latents": a.lat, "dtype": "fp16", "sampler": "dpm",
              "guidance_scale": GUIDANCE, "context": CONTEXT, "windows_per_step": windows,
              "step_plain_16_frames": stats(times["plain"]), "step_windowed": stats(times["windowed"]),
              "windows_times_plain_ms": round(windows * plain, 4),
              "windowed_minus_windows_times_plain_ms": round(windowed - windows * plain, 4),
              "difference_per_window_ms": round((windowed - windows * plain) / windows, 4),
              "difference_percent_of_windows_times_plain": round(100 * (windowed - windows * plain) / (windows * plain), 3),
              "gather_launch_eager": stats(launches["window_gather_latents"]), "merge_launch_eager": stats(launches["window_merge_tokens"]),
              "bytes_per_window_mbytes": {"gather": round(2 * 4 * CONTEXT["frames"] * hw * 4 / 1e6, 2),
                                          "merge_tokens_read": round(2 * CONTEXT["frames"] * hw * 8 / 1e6, 2),
                                          "merge_acc_or_merged": round(CONTEXT["frames"] * hw * 16 / 1e6, 2)},
              "note": "three plain steps hold three solver kernels over 16 frames, the windowed step one over 32: the difference per window "
                      "is gather + merge less a third of that saving"}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
