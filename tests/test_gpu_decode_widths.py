"""The decode step (`afhip_llm_decode_step`) at every width the imaged phases accept, against the float64 step of tests/decode_ref.py.

Each model is the recipe of helpers.build_wide_llm (seeded weights on the CPU, rounded to bf16 once, 2 layers) at a smaller width and a
20 000-id text vocabulary.  Every step is judged on its own: the reference reads the device's own cache and previous tokens.  The widths
reach what the AF3-7B shape does not: few tile rows per unit, idle workgroups, hd 64 in the imaged attention, e4m3 K / 128 = 8 exactly and
split 2 / 1 over the waves, the predicate's edges; H 512 in W8A16 is sent to the row-major launches (e4m3 K < 1024), and the Qwen2-1.5B
width (inter 8960, not a multiple of 512) and the Qwen2-0.5B width (H 896) never take the imaged path.  Tolerances: tests/decode_ref.py (KV bounds, pick_eps)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import decode_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TEXT_VOCAB = 20000
N_STEPS = 4
SENTINEL = 0x4B3D            # bf16 12 160: no cache row the step must not touch may change
# (H, inter, n_q, n_kv) -> imaged in bf16, imaged in W8A16 (on 256 CUs)
SHAPES = {
    (512, 4096, 8, 2): (True, False),           # TR 2, 64 idle q|k|v workgroups; e4m3 K = 512 -> row-major launches
    (1024, 4096, 8, 1): (True, True),           # GQA rep 8, e4m3 K / 128 = 8 exactly
    (1536, 8704, 12, 2): (True, True),          # e4m3 steps split 2 / 1 over the waves, TR 6 / 4
    (2048, 5632, 32, 4): (True, True),          # hd 64 imaged attention, TR 8 / 5
    (4096, 4096, 64, 32): (True, True),         # cdiv(H, 256) = 16, cdiv(qw, 256) = 32
    (1536, 8960, 12, 2): (False, False),        # Qwen2-1.5B: 8960 % 512 != 0
    (896, 4864, 14, 2): (False, False),         # Qwen2-0.5B: H % 512 != 0, q|k|v 1152, hd 64
}
# >= 6 sorted disjoint intervals: single ids, one across the 64-row lm_head unit boundary at 128, the last end not a multiple of 64
INTERVALS = [[3, 4], [7, 8], [100, 130], [300, 2000], [2500, 9000], [12000, 20131]]
HEAD_ROWS = 20131


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")


def _opt(name, value):
    from audio_intelligence_amd import _lib as L
    L.check(L.lib().afhip_set_option(name.encode(), int(value)))


@pytest.fixture(autouse=True)
def _imaged_on():
    yield
    if torch.cuda.is_available():
        _opt("DECODE_IMAGED", 1)


@pytest.fixture(scope="module", params=list(SHAPES), ids=lambda s: "H%d_I%d_q%d_kv%d" % s)
def wide(request):
    _need_gpu()
    torch.set_num_threads(H.cpu_threads())
    model, sd, cfg = H.build_llm_at(request.param, TEXT_VOCAB)
    refs = {"bf16": sd}
    yield request.param, model, refs, cfg
    del model, refs
    torch.cuda.empty_cache()


def _mode(model, refs, sd_bf16, mode):
    model.enable_fp8_decode(mode == "w8a16")
    if mode not in refs:
        refs[mode] = R.dequantize_e4m3(sd_bf16, device=DEV)[0]          # quantised where pack_qwen2_weights quantises
    return refs[mode]


def _imaged(model, B, cap):
    from audio_intelligence_amd import _lib as L
    return L.lib().afhip_llm_decode_imaged(C.byref(model.pack(cap).w), B)


def _history(model, cfg, B, T0, seed):
    """a cache for B + 2 sequences: positions [0, T0) of the first B hold seeded bf16 rows at the model's K / V scale (q / k weights
    0.06, v 0.02, unit-rms normed input: 0.06 sqrt(H) and 0.02 sqrt(H)), everything else the sentinel"""
    cache = model.new_cache(B + 2, T0 + N_STEPS + 4)
    Hd = cfg["hidden_size"]
    g = torch.Generator().manual_seed(seed)
    L_, _, nkv, _, hd = cache.k.shape
    kh = (torch.randn(L_, B, nkv, T0, hd, generator=g) * 0.06 * Hd ** 0.5).to(torch.bfloat16)
    vh = (torch.randn(L_, B, nkv, T0, hd, generator=g) * 0.02 * Hd ** 0.5).to(torch.bfloat16)
    for t in (cache.k, cache.v):
        t.view(torch.int16).fill_(SENTINEL)
    cache.k[:, :B, :, :T0] = kh.to(DEV)
    cache.v[:, :B, :, :T0] = vh.to(DEV)
    cache.length = T0
    return cache


def _prev_tokens(B, seed):
    rng = np.random.default_rng(seed)
    ids = [i for lo, hi in INTERVALS for i in range(lo, hi)]
    return torch.tensor(rng.choice(ids, size=B), dtype=torch.int64)


def _decode(model, cache, prev, B, T0, head_rows, n_steps=N_STEPS):
    """n_steps eager decode steps as _greedy_device_loop.one_step issues them; yields (step, cache rows before the step, prev before)"""
    pk = model.pack(cache.cap)
    prev = prev.to(DEV).clone()
    out = torch.zeros((n_steps, B), dtype=torch.int64, device=DEV)
    finished = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    seq_pos = torch.full((B,), T0, dtype=torch.int32, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    iv = torch.tensor(INTERVALS, dtype=torch.int32, device=DEV)
    ws = model._workspace(B, 1, cache.cap)
    for step in range(n_steps):
        kb, vb, pb = cache.k[:, :B].cpu(), cache.v[:, :B].cpu(), prev.cpu()
        torch.ops.afhip.llm_decode_step(pk.blob, cache.k, cache.v, prev, out, finished, iv, -1, -1, seq_pos, counter, T0 + n_steps - 1, ws, head_rows)
        torch.cuda.synchronize()
        yield step, kb, vb, pb, out


def _run_case(shape, model, sd, cfg, mode, B, T0, path, report):
    Hd = shape[0]
    expect = SHAPES[shape][mode == "w8a16"] and path == "imaged"
    _opt("DECODE_IMAGED", 1 if path == "imaged" else 0)
    cache = _history(model, cfg, B, T0, seed=Hd + B)
    assert _imaged(model, B, cache.cap) == int(expect), f"{shape} {mode} B={B}: afhip_llm_decode_imaged != {int(expect)}"
    k0, v0 = cache.k.clone(), cache.v.clone()
    prev = _prev_tokens(B, seed=B + T0)
    worst = {}
    ids = None
    for step, kb, vb, pb, out in _decode(model, cache, prev, B, T0, HEAD_ROWS):
        pos = T0 + step
        ref = R.decode_step(sd, cfg, pb, torch.full((B,), pos), kb, vb, INTERVALS, head_rows=HEAD_ROWS, n_stream=model.num_stream)
        for name, got, want in (("K", cache.k, ref.k), ("V", cache.v, ref.v)):
            hip = got[:, :B, :, pos].cpu()
            assert bool(torch.isfinite(hip.float()).all()), (name, step)
            mx, mn = R.kv_error(hip, want)                                 # [L, B]
            for l in range(mx.shape[0]):
                bmax, bmean = R.kv_bounds(l, Hd, mode == "w8a16")
                w = worst.setdefault((name, l), [0.0, 0.0])
                w[0], w[1] = max(w[0], float(mx[l].max())), max(w[1], float(mn[l].max()))
                assert float(mx[l].max()) <= bmax and float(mn[l].max()) <= bmean, \
                    f"{shape} {mode} {path} B={B} T0={T0} step {step}: layer {l} {name} row e max {float(mx[l].max()):.2f} mean {float(mn[l].max()):.3f} > {(bmax, bmean)}"
        pick = out[step].cpu()
        eps = R.pick_eps(ref.logits)
        for b in range(B):
            p = int(pick[b])
            assert any(lo <= p < hi for lo, hi in INTERVALS), f"step {step} seq {b}: id {p} not allowed"
            regret = float(ref.logits[b].max() - ref.logits[b, p])
            assert regret <= float(eps[b]), f"{shape} {mode} {path} B={B} step {step} seq {b}: regret {regret:.4f} > {float(eps[b]):.4f}"
            if float(ref.margin[b]) > float(eps[b]):
                assert p == int(ref.pick[b]), f"{shape} {mode} {path} B={B} step {step} seq {b}: {p} != f64 argmax {int(ref.pick[b])}"
        ids = out.cpu()
    # nothing outside the appended rows changed: the history, the rows past the last step, the two sequences past the batch
    t1 = T0 + N_STEPS
    for got, before in ((cache.k, k0), (cache.v, v0)):
        assert torch.equal(got[:, :B, :, :T0].view(torch.int16), before[:, :B, :, :T0].view(torch.int16)), "history rows changed"
        assert bool((got[:, :B, :, t1:].view(torch.int16) == SENTINEL).all()), "rows past the appended positions changed"
        assert bool((got[:, B:].view(torch.int16) == SENTINEL).all()), "sequences past the batch changed"
    report.append((shape, mode, path if expect else "fallback", B, T0, worst))
    print(f"{shape} {mode} {path}->{'imaged' if expect else 'fallback'} B={B} T0={T0}: " +
          ", ".join(f"L{l}{n} {w[0]:.2f}/{w[1]:.3f}" for (n, l), w in sorted(worst.items(), key=lambda kv: (kv[0][1], kv[0][0]))))
    return ids


CASES = [("imaged", B) for B in (1, 8, 9, 16)] + [("fallback", B) for B in (1, 9)]


@pytest.mark.parametrize("mode", ["bf16", "w8a16"])
def test_decode_step_matches_f64_reference(wide, mode):
    """per case: the expected path (afhip_llm_decode_imaged), the appended K/V rows of both layers within decode_ref's bounds of the
    float64 step, every pick allowed and within pick_eps of the best float64 logit (the argmax when the margin exceeds it), the rest of
    the cache untouched; head_rows = the last interval end and head_rows = 0 give the same ids"""
    shape, model, refs, cfg = wide
    sd = _mode(model, refs, refs["bf16"], mode)
    report = []
    for path, B in CASES:
        T0 = 126 if B in (8, 9) else 37                         # 126: the 4 steps cross the 128-key range
        ids = _run_case(shape, model, sd, cfg, mode, B, T0, path, report)
        if B == 9:
            cache = _history(model, cfg, B, T0, seed=shape[0] + B)
            for step, *_, out in _decode(model, cache, _prev_tokens(B, seed=B + T0), B, T0, 0):
                pass
            assert torch.equal(out.cpu(), ids), f"{shape} {mode} {path}: head_rows 0 and {HEAD_ROWS} give different ids"


@pytest.mark.parametrize("mode", ["bf16", "w8a16"])
@pytest.mark.parametrize("row", ["shared", "zero"])
def test_decode_step_tied_logits_pick_smallest_allowed_id(wide, mode, row):
    """every allowed lm_head row set to one shared vector (or zero): all allowed logits are bit-identical, spread over every workgroup of
    the lm_head phase; the pick is the smallest allowed id, on both paths"""
    shape, model, refs, cfg = wide
    model.enable_fp8_decode(mode == "w8a16")
    w = model.lm_head.weight
    saved = w.detach().clone()
    try:
        with torch.no_grad():
            v = torch.zeros_like(w[0]) if row == "zero" else saved[INTERVALS[3][0] + 5].clone()
            for lo, hi in INTERVALS:
                w[lo:hi] = v
        model._packed = None
        for path in ("imaged", "fallback"):
            _opt("DECODE_IMAGED", 1 if path == "imaged" else 0)
            B = 9
            cache = _history(model, cfg, B, 37, seed=7)
            for step, *_, out in _decode(model, cache, _prev_tokens(B, seed=1), B, 37, HEAD_ROWS, n_steps=2):
                pass
            assert out.cpu().eq(INTERVALS[0][0]).all(), f"{shape} {mode} {path} {row}: tied picks {out.cpu().tolist()}"
    finally:
        with torch.no_grad():
            w.copy_(saved)
        model._packed = None


@pytest.mark.parametrize("shape_mode", [((1024, 4096, 8, 1), "bf16"), ((2048, 5632, 32, 4), "w8a16")])
def test_decode_step_batch_invariance(wide, shape_mode):
    """a sequence decoded alone gives the same bits -- appended K/V rows and ids -- as inside a batch of 9 (RM 16 image) and of 16"""
    shape, model, refs, cfg = wide
    if shape != shape_mode[0]:
        pytest.skip("batch invariance runs at one width per mode")
    model.enable_fp8_decode(shape_mode[1] == "w8a16")
    T0 = 37
    for Bb in (9, 16):
        cache = _history(model, cfg, Bb, T0, seed=11)
        prev = _prev_tokens(Bb, seed=12)
        for step, *_, out in _decode(model, cache, prev, Bb, T0, HEAD_ROWS):
            pass
        ids_b, k_b, v_b = out.cpu(), cache.k.cpu(), cache.v.cpu()
        for b in (0, 4, Bb - 1):
            c1 = model.new_cache(1 + 2, T0 + N_STEPS + 4)
            for t in (c1.k, c1.v):
                t.view(torch.int16).fill_(SENTINEL)
            c1.k[:, :1, :, :T0] = k_b[:, b:b + 1, :, :T0].to(DEV)
            c1.v[:, :1, :, :T0] = v_b[:, b:b + 1, :, :T0].to(DEV)
            for step, *_, out1 in _decode(model, c1, prev[b:b + 1], 1, T0, HEAD_ROWS):
                pass
            assert out1.cpu()[:, 0].tolist() == ids_b[:, b].tolist(), f"B={Bb} seq {b}: alone {out1.cpu()[:, 0].tolist()} != batched {ids_b[:, b].tolist()}"
            for got, want in ((c1.k, k_b), (c1.v, v_b)):
                assert torch.equal(got[:, 0, :, T0:T0 + N_STEPS].cpu().view(torch.int16), want[:, b, :, T0:T0 + N_STEPS].view(torch.int16)), f"B={Bb} seq {b}: K/V bits"


def test_decode_loop_graph_replay_matches_eager(wide, monkeypatch):
    """_greedy_device_loop over 20 steps with the hipGraph replay on and off: identical ids and cache bits (smallest width)"""
    shape, model, refs, cfg = wide
    if shape != (512, 4096, 8, 2):
        pytest.skip("graph replay runs at the smallest width")
    model.enable_fp8_decode(False)
    res = []
    for g in ("1", "0"):
        monkeypatch.setenv("AFHIP_DECODE_GRAPH", g)
        cache = _history(model, cfg, 3, 37, seed=5)
        tok = model.text_token.expand(3, -1, -1).clone()
        model.eos_token_id = model.eot_token_id = -1
        hyp, _, cache = model._greedy_device_loop(tok, cache, "text", 20, poll=10 ** 9)
        res.append((hyp.cpu(), cache.k.cpu(), cache.v.cpu()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1].view(torch.int16), res[1][1].view(torch.int16)) and torch.equal(res[0][2].view(torch.int16), res[1][2].view(torch.int16))
