"""A/B of the denoising step with guidance_rescale off and on at the metric configuration (fp16, 16 frames of 64x64 latents, guidance 9,
hipGraph replay, DPM-Solver++): one seeded v1.02 UNet, `LatentToVideoPipeline.denoise` run alternately without and with
`guidance_rescale`, a device event recorded in the per-step callback - the time between two callbacks is one step: session replay,
(aa_cfg_rescale_tokens,) the solver kernel.  Then the two launches of aa_cfg_rescale_tokens alone, between their own pair of events.

    python scripts/bench_guidance_rescale.py [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/guidance_rescale_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GUIDANCE, RESCALE = 9.0, 0.7


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

    def run(rescale):
        """One denoise call; returns the milliseconds between consecutive callbacks behind the warm-up."""
        marks = []

        def mark(i, t, x):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append(e)
        pipe.denoise(inp["latents"].clone(), embeds, inp["cond"], inp["mask"], [3.0], ts, GUIDANCE, callback=mark, guidance_rescale=rescale)
        torch.cuda.synchronize()
        return [marks[k].elapsed_time(marks[k + 1]) for k in range(a.warmup, len(marks) - 1)]

    times = {"off": [], "on": []}
    with torch.no_grad():
        run(0.0), run(RESCALE)                                    # capture, tile choices, workspaces
        for _ in range(a.rounds):                                 # alternately, so drift of the clocks hits both alike
            times["off"] += run(0.0)
            times["on"] += run(RESCALE)
        # the two launches alone, between their own events
        real, pairs = ops.cfg_rescale_tokens, []

        def timed(*x, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = real(*x, **k)
            e1.record()
            pairs.append((e0, e1))
            return out
        ops.cfg_rescale_tokens = timed
        try:
            run(RESCALE)
        finally:
            ops.cfg_rescale_tokens = real
        launches = [e0.elapsed_time(e1) for e0, e1 in pairs[a.warmup:]]
    off_med, on_med = statistics.median(times["off"]), statistics.median(times["on"])
    rows = 2 * (a.frames + 1) * a.lat * a.lat
    result = {"what": "one guided denoising step (UNet graph replay + solver kernel), guidance_rescale off / on, runs alternated",
              "device": torch.cuda.get_device_name(0), "frames": a.frames, "latents": a.lat, "dtype": "fp16", "sampler": "dpm",
              "guidance_scale": GUIDANCE, "guidance_rescale": RESCALE,
              "step_off": stats(times["off"]), "step_on": stats(times["on"]),
              "on_minus_off_ms": round(on_med - off_med, 4), "on_minus_off_percent_of_step": round(100 * (on_med - off_med) / off_med, 3),
              "cfg_rescale_two_launches_eager": stats(launches),
              "token_matrix_mbytes": round(rows * 8 * 2 / 1e6, 2),
              "note": "the pair reads frames 1..T of both halves twice (moments, apply) and writes the unconditional half once; the "
                      "solver kernel behind it then reads one half instead of two"}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
