"""Device-event timing of afhip_sample_filter (one call = every launch of the filter-and-draw) at V = 152 064 for B in {1, 8, 16, 32}:
  hf    T 0.7, top-k 20, top-p 0.8, repetition penalty 1.05 over 512 ids per row
  top_p top-p 0.95 only
  ualm  exact top-k 1000 over 8 streams per sequence (rows = 8 B) with the guidance mix, cfg 3, and per-stream id intervals
Prints one JSON line per (config, B): median and min device microseconds per call (hipGraph replay of one call) over --iters
replays, and the mean per call when called eagerly from Python (us_eager)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_intelligence_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--V", type=int, default=152064)
    ap.add_argument("--batches", default="1,8,16,32")
    a = ap.parse_args()
    dev = "cuda:0"
    V = a.V
    for B in [int(x) for x in a.batches.split(",")]:
        for name in ("hf", "top_p", "ualm"):
            rows = 8 * B if name == "ualm" else B
            g = torch.Generator(device=dev).manual_seed(B)
            lg = torch.randn(rows, V, device=dev, generator=g) * 3
            u = torch.rand(rows, device=dev, generator=g)
            kw = {}
            if name == "hf":
                ids = torch.randint(0, V, (rows, 512), device=dev, dtype=torch.int32, generator=g)
                kw = dict(temperature=0.7, top_k=20, top_p=0.8, penalty=1.05, penalty_ids=ids,
                          n_ids=torch.full((rows,), 512, dtype=torch.int32, device=dev))
            elif name == "top_p":
                kw = dict(top_p=0.95)
            else:
                cl = torch.randn(rows, V, device=dev, generator=g) * 3
                w = V // 8
                iv = torch.tensor([[[s * w, (s + 1) * w]] for s in range(8)] * B, dtype=torch.int32, device=dev)
                kw = dict(temperature=0.8, top_k=1000, exact_k=True, allowed=iv, cfg_logits=cl, cfg=3.0)
            for _ in range(3):
                ops.sample_filter(lg, u=u, **kw)
            torch.cuda.synchronize()
            # device time: the call captured once in a hipGraph and replayed, so no host work sits between the events
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ops.sample_filter(lg, u=u, **kw)
            ts = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1000.0)
            # eager: one Python call per step (argument checks, workspace allocation and the launches from the host)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                ops.sample_filter(lg, u=u, **kw)
            e1.record()
            e1.synchronize()
            eager = e0.elapsed_time(e1) * 1000.0 / a.iters
            ts.sort()
            print(json.dumps({"config": name, "B": B, "rows": rows, "V": V, "us_median": round(ts[len(ts) // 2], 2),
                              "us_min": round(ts[0], 2), "us_eager": round(eager, 2), "iters": a.iters}), flush=True)


if __name__ == "__main__":
    main()
