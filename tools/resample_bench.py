#!/usr/bin/env python3
"""Times the GPU resampler (afhip_resample) on B x 30 s batches -> 16 kHz with device events and prints one JSON line per input rate:
us per batch, GFLOP/s (2 x taps x outputs; taps = the non-zero ones, 2K+1), fraction of the 157.3 TF fp32 peak, and effective GB/s
(input read once + output written once).  usage: python tools/resample_bench.py [--batch 32] [--rates 44100,48000] [--iters 50]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from audio_intelligence_amd.multimodal_io import resample as RS  # noqa: E402

PEAK_F32 = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rates", default="44100,48000")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a HIP device")
    res = []
    for fs in [int(r) for r in a.rates.split(",")]:
        n_in = 30 * fs
        x = torch.randn((a.batch, n_in), device="cuda") * 0.1
        n_out = RS.out_length(n_in, fs, 16000)
        for _ in range(a.warmup):
            RS.resample_device(x, fs, 16000, n_out=n_out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            RS.resample_device(x, fs, 16000, n_out=n_out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.iters
        _, _, K, _ = RS.plan(fs, 16000)
        flop = 2.0 * (2 * K + 1) * n_out * a.batch
        nbytes = 4.0 * a.batch * (n_in + n_out)
        res.append({"fs_in": fs, "batch": a.batch, "seconds": 30, "us": round(us, 1), "gflops": round(flop / us / 1e3, 1),
                    "frac_f32_peak": round(flop / (us * 1e-6) / PEAK_F32, 3), "eff_gbs": round(nbytes / us / 1e3, 1)})
    print(json.dumps({"resample": res, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
