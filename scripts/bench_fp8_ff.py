"""The FeedForward + proj_out tail of a wide transformer, 16-bit chain against the opt-in e4m3 chain, at the three real shape sets of the
[2,4,16,64,64] step (tokens, C) = (34816, 640), (8704, 1280), (2176, 1280).  Same process, interleaved, device events, median of the repeats.

  16-bit: LayerNorm kernel -> GEGLU contraction -> merged (ff-out + residual | proj_out + outer) contraction       (3 launches; inside the step the
          LayerNorm is folded into the GEGLU contraction from producer-written statistics, so this side carries one small kernel more than the step)
  e4m3:   quantise (LayerNorm inside) -> GEGLU contraction -> quantise -> ff-out contraction + residual -> proj_out contraction + outer (5 launches)

TF/s count the multiply-adds of the three linear maps (2 M C (8C + 4C + C)) over the chain's time.  Needs the MI355X."""
import argparse
import json
import statistics

import torch

from animate_anything_amd import layers

SHAPES = [(34816, 640), (8704, 1280), (2176, 1280)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fp8_ff.py measures on the GPU only"
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    rows = []
    for M, C in SHAPES:
        torch.manual_seed(C)
        tr = layers.Transformer2DModel(C // 64, 64, C).eval().to(dt).cuda()
        blk = tr.transformer_blocks[0]
        g = torch.Generator(device="cuda").manual_seed(M)
        x = torch.randn(M, C, generator=g, device="cuda").to(dt)
        outer = torch.randn(M, C, generator=g, device="cuda").to(dt)
        mt = tr.merged_tail()
        assert mt is not None

        def chain16():
            return blk.ff.tokens(blk.norm3.tokens(x), residual=x, tail=(mt, outer))

        def chain8():
            return tr.proj_out.tokens(blk.ff.tokens_fp8(x, blk.norm3, residual=x), residual=outer)

        with torch.no_grad():
            for _ in range(a.warmup):
                y16, y8 = chain16(), chain8()
            torch.cuda.synchronize()
            diff = (y16.float() - y8.float()).abs().max().item() / max(1.0, y16.float().abs().max().item())
            t = {"fp16": [], "fp8": []}
            for _ in range(a.repeats):                     # interleaved: both see the same clocks and the same neighbours
                for name, fn in (("fp16", chain16), ("fp8", chain8)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    t[name].append(e0.elapsed_time(e1) * 1e3)
        flop = 2.0 * M * C * 13 * C
        row = {"tokens": M, "channels": C, "dtype": a.dtype, "repeats": a.repeats, "max_diff_rel_range": diff}
        for name in t:
            med = statistics.median(t[name])
            row[name + "_us"] = round(med, 1)
            row[name + "_us_min_max"] = [round(min(t[name]), 1), round(max(t[name]), 1)]
            row[name + "_tflops"] = round(flop / med / 1e6, 1)
        row["fp8_over_fp16_time"] = round(row["fp8_us"] / row["fp16_us"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
