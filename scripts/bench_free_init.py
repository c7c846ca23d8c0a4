"""One FreeInit re-initialisation (ops.freeinit_mix: five launches, direct DFTs over frames x h x w) next to one guided denoising step
at the metric configuration (fp16 UNet, 16 frames of 64x64 latents, guidance batch 2, hipGraph replay), timed alternately in one process
with device events; the mix also checked against float64 torch.fft on the CPU.  The mix runs num_iters - 1 times per SAMPLE, the step
num_iters * num_inference_steps times.

    python scripts/bench_free_init.py [--steps 20] [--warmup 5] [--clips 2] [--out profiles/free_init.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FREE_INIT = dict(method="butterworth", order=4, spatial_stop_frequency=0.25, temporal_stop_frequency=0.25)
A, S = 0.068, 0.998                                              # sqrt(abar), sqrt(1 - abar) at t = 999 of the scaled-linear schedule


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--clips", type=int, default=2)
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--lat", type=int, default=64)
    p.add_argument("--no-unet", action="store_true", help="time the mix alone")
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert a.steps >= 20 and a.warmup >= 5, "at least 5 warm-up and 20 timed steps"
    import bench
    from animate_anything_amd import ops
    from animate_anything_amd.schedulers import free_init_filter
    from util import fullsize_inputs
    dev = torch.device("cuda:0")
    T, h, w = a.frames, a.lat, a.lat
    g = torch.Generator().manual_seed(3)
    x, n0, z = (torch.randn(a.clips, 4, T, h, w, generator=g) for _ in range(3))
    tables = ops.free_init_tables(T, h, w, free_init_filter(T, h, w, **FREE_INIT), dev)
    xd, nd, zd = x.to(dev), n0.to(dev), z.to(dev)
    out = torch.empty_like(xd)
    mix = lambda: ops.freeinit_mix(xd, nd, zd, A, S, tables, out=out)
    step = None
    if not a.no_unet:
        net = bench.build_unet(torch.float16, dev)
        i = fullsize_inputs(a.frames, a.lat)
        hf = lambda t: t.half().to(dev)
        args = (hf(i["sample"]), i["t"], hf(i["text"]), hf(i["cond"]), hf(i["mask"]))
        net.enable_graph()
        step = lambda: net(*args, motion=i["motion"])
    times = {"mix": [], "step": []}
    with torch.no_grad():
        for k in range(a.warmup + a.steps):                      # alternately, so drift of the clocks hits both alike
            for name, fn in (("mix", mix), ("step", step)):
                if fn is None:
                    continue
                ms = timed(fn)
                if k >= a.warmup:
                    times[name].append(ms)
    dims = (-3, -2, -1)
    a32, s32 = float(torch.tensor(A, dtype=torch.float32)), float(torch.tensor(S, dtype=torch.float32))
    d = a32 * x.double() + s32 * n0.double() - z.double()
    lp = torch.fft.ifftn(tables.mask.double().cpu() * torch.fft.fftn(d, dim=dims), dim=dims).real
    err = (out.double().cpu() - (z.double() + lp)).abs().max().item()
    n = x.numel()
    launches = [("rows forward (w)", 3 * 4 * n, 8 * n), ("axis forward (h)", 8 * n, 8 * n), ("frames forward, mask, inverse", 8 * n + 4 * n, 8 * n),
                ("axis inverse (h)", 8 * n, 8 * n), ("rows inverse (w), + z", 8 * n + 4 * n, 4 * n)]
    result = {"what": "one FreeInit re-initialisation (ops.freeinit_mix, five launches) next to the UNet forward of one guided denoising step "
                      "(graph replay), timed alternately",
              "device": torch.cuda.get_device_name(0), "clips": a.clips, "channels": 4, "frames": T, "latents": a.lat, "free_init": FREE_INIT,
              "mix": stats(times["mix"]), "step": stats(times["step"]) if times["step"] else None,
              "mix_percent_of_step": round(100 * statistics.median(times["mix"]) / statistics.median(times["step"]), 3) if times["step"] else None,
              "max_abs_error_against_float64_fft": err, "lp_max_abs": lp.abs().max().item(),
              "launches": [dict(launch=name, mbytes_read=round(r / 1e6, 2), mbytes_written=round(wr / 1e6, 2)) for name, r, wr in launches],
              "mbytes_moved_total": round(sum(r + wr for _, r, wr in launches) / 1e6, 2),
              "note": "bytes per launch from the geometry: fp32 operands, the complex fp32 workspace in place; the mask (4 bytes per element of "
                      "one volume) is re-read per volume and counted once per element"}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
