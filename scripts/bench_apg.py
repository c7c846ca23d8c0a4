"""A/B of the denoising step with Adaptive Projected Guidance off and on at the metric configuration (fp16, 16 frames of 64x64 latents,
guidance 9, hipGraph replay, DPM-Solver++): one seeded v1.02 UNet, `LatentToVideoPipeline.denoise` run alternately without `apg` (the
path of before), with it (momentum off) and with it and a momentum buffer, a device event recorded in the per-step callback - the time
between two callbacks is one step: session replay, (aa_apg_tokens,) the solver kernel.  Then the two launches of aa_apg_tokens alone,
between their own pair of events, without and with momentum.

    python scripts/bench_apg.py [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/apg_ab.json]
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
VARIANTS = {"off": None, "on": dict(eta=0.0, norm_threshold=30.0, momentum=0.0), "on_momentum": dict(eta=0.0, norm_threshold=30.0, momentum=-0.5)}


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20, help="timed steps per variant, spread over the rounds")
    p.add_argument("--warmup", type=int, default=5, help="untimed steps in front of every run")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--lat", type=int, default=64)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert a.steps >= 20 and a.warmup >= 5, "at least 5 warm-up and 20 timed steps"
    import bench
    from animate_anything_amd import ops
    from animate_anything_amd.pipeline import LatentToVideoPipeline
    from animate_anything_amd.schedulers import DPMSolverMultistepScheduler
    dev = torch.device("cuda:0")
    unet = bench.build_unet(torch.float16, dev)
    unet.enable_graph()
    pipe = LatentToVideoPipeline(vae=None, unet=unet, scheduler=DPMSolverMultistepScheduler())
    inp = bench.synthetic_inputs(a.frames, a.lat, torch.float16, dev)
    embeds = torch.cat([inp["neg"], inp["text"]])
    per_round = -(-a.steps // a.rounds)
    pipe.scheduler.set_timesteps(a.warmup + per_round + 1)
    ts = [int(t) for t in pipe.scheduler.timesteps][:a.warmup + per_round + 1]

    def run(apg):
        """One denoise call; returns the milliseconds between consecutive callbacks behind the warm-up."""
        marks = []

        def mark(i, t, x):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append(e)
        pipe.denoise(inp["latents"].clone(), embeds, inp["cond"], inp["mask"], [3.0], ts, GUIDANCE, callback=mark, apg=apg)
        torch.cuda.synchronize()
        return [marks[k].elapsed_time(marks[k + 1]) for k in range(a.warmup, len(marks) - 1)]

    times = {name: [] for name in VARIANTS}
    launches = {}
    with torch.no_grad():
        for apg in VARIANTS.values():                             # capture, tile choices, workspaces
            run(apg)
        for _ in range(a.rounds):                                 # alternately, so drift of the clocks hits all alike
            for name, apg in VARIANTS.items():
                times[name] += run(apg)
        # the two launches alone, between their own events
        real = ops.apg_tokens
        for name in ("on", "on_momentum"):
            pairs, clipped = [], torch.zeros(2, dtype=torch.float32, device=dev)

            def timed(*x, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = real(*x, stats=clipped, **k)
                e1.record()
                pairs.append((e0, e1))
                return out
            ops.apg_tokens = timed
            try:
                run(VARIANTS[name])
            finally:
                ops.apg_tokens = real
            launches[name] = stats([e0.elapsed_time(e1) for e0, e1 in pairs[a.warmup:]])
            launches[name]["last_step_s_p"] = [round(v, 5) for v in clipped.tolist()]
    med = {name: statistics.median(ms) for name, ms in times.items()}
    rows = 2 * (a.frames + 1) * a.lat * a.lat
    result = {"what": "one guided denoising step (UNet graph replay + solver kernel), apg off / on / on with momentum, runs alternated",
              "device": torch.cuda.get_device_name(0), "frames": a.frames, "latents": a.lat, "dtype": "fp16", "sampler": "dpm",
              "guidance_scale": GUIDANCE, "apg": {k: v for k, v in VARIANTS.items() if v is not None},
              "step_off": stats(times["off"]), "step_on": stats(times["on"]), "step_on_momentum": stats(times["on_momentum"]),
              "on_minus_off_ms": round(med["on"] - med["off"], 4), "on_minus_off_percent_of_step": round(100 * (med["on"] - med["off"]) / med["off"], 3),
              "on_momentum_minus_off_ms": round(med["on_momentum"] - med["off"], 4),
              "on_momentum_minus_off_percent_of_step": round(100 * (med["on_momentum"] - med["off"]) / med["off"], 3),
              "apg_two_launches_eager": launches["on"], "apg_two_launches_eager_momentum": launches["on_momentum"],
              "token_matrix_mbytes": round(rows * 8 * 2 / 1e6, 2),
              "momentum_buffer_mbytes": round(a.frames * a.lat * a.lat * 4 * 4 / 1e6, 2),
              "note": "the pair reads frames 1..T of both halves twice (moments, apply) and writes the unconditional half once; with momentum "
                      "the fp32 buffer is read and written by the first launch and read by the second, which then reads one half; the solver "
                      "kernel behind it reads one half instead of two.  The UNet's weights are seeded, not trained: (s, p) say nothing about "
                      "a real checkpoint."}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
