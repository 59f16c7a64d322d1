"""Device-event timing of the two beam-search kernels at the 7B shape (V = 152 064, 28 layers, 4 kv heads, head_dim 128, bf16).
  beam_select  afhip_beam_select (3 launches) against the torch path it replaces -- log_softmax + add + topk over nb x V -- on the
               same inputs, for R = B x nb in {4, 8, 16, 32} rows (nb = 4, K = 2 nb); the two must select the same index sets first
  kv_gather    afhip_kv_gather in place over 128 generated rows per slot at R = 8, for a map that moves 3 of 4 beams of each prompt
               from one parent (no staging) and for swaps (every moved slot staged)
Prints one JSON line per measurement: mean device microseconds per call over --iters calls issued back to back."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_intelligence_amd import ops  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    dev = "cuda:0"
    V, nb = 152064, 4
    K = 2 * nb
    for R in (4, 8, 16, 32):
        B = R // nb
        g = torch.Generator(device=dev).manual_seed(R)
        lg = (torch.randn(R, V, device=dev, generator=g) * 3).bfloat16().float()
        run = -torch.rand(B, nb, device=dev, generator=g) * 5

        def torch_path():
            acc = (torch.log_softmax(lg, -1).view(B, nb, V) + run[:, :, None]).reshape(B, nb * V)
            return torch.topk(acc, K)

        tv, ti = torch_path()
        hv, hi = ops.beam_select(lg, run, K, model_dtype=torch.bfloat16)
        # torch's log_softmax sums in its own order: values may differ by an ulp, so neighbours that close may swap places
        same = bool(torch.equal(torch.sort(ti, -1)[0], torch.sort(hi, -1)[0])) and bool(((tv - hv).abs() <= 1e-5 * tv.abs().clamp(min=1)).all())
        if not same:
            raise SystemExit(f"beam_select and the torch path disagree at R = {R}: {ti.tolist()} vs {hi.tolist()}")
        us_h = timed(lambda: ops.beam_select(lg, run, K, model_dtype=torch.bfloat16), a.iters)
        us_t = timed(torch_path, a.iters)
        print(json.dumps({"probe": "beam_select", "R": R, "V": V, "K": K, "equal_index_sets": same, "equal_order": bool(torch.equal(ti, hi)), "us_hip": round(us_h, 2),
                          "us_torch": round(us_t, 2), "bytes_read": 2 * R * V * 4}), flush=True)
    n_l, nkv, hd, R, cap, rows = 28, 4, 128, 8, 512, 128
    k = torch.randn(n_l, R, nkv, cap, hd, device=dev).bfloat16()
    v = torch.randn_like(k)
    row0 = torch.full((R,), 200, dtype=torch.int32, device=dev)
    row1 = row0 + rows
    ws = None
    for name, par in (("three-from-one", [0, 0, 0, 0, 4, 4, 4, 4]), ("swaps", [1, 0, 3, 2, 5, 4, 7, 6])):
        parent = torch.tensor(par, dtype=torch.int32, device=dev)
        ws = ops.kv_gather(k, v, k, v, parent, row0, row1, rows, ws=ws)
        us = timed(lambda: ops.kv_gather(k, v, k, v, parent, row0, row1, rows, ws=ws), a.iters)
        moved = sum(int(p != r) for r, p in enumerate(par))
        staged = sum(int(p != r and par[p] != p) for r, p in enumerate(par))
        per_slot = n_l * nkv * rows * hd * 2 * 2
        print(json.dumps({"probe": "kv_gather", "map": name, "R": R, "rows": rows, "moved_slots": moved, "staged_slots": staged,
                          "bytes_copied": (moved + staged) * per_slot, "us": round(us, 2)}), flush=True)


if __name__ == "__main__":
    main()
