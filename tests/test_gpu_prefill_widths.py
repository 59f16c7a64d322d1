"""The multi-token forward (`afhip_llm_forward`, T > 1, any pos0) and the per-sequence-position step (`afhip_llm_forward_ragged`) at every
width of tests/test_gpu_decode_widths.py plus Qwen2-0.5B (896 / 4864 / 14:2), against the float64 forward of tests/prefill_ref.py.

Each model is helpers.build_llm_at's recipe (2 layers, bf16).  Every appended K/V row and every hidden row is judged against
prefill_ref.row_bounds; every cache row outside the rows a call appends must keep the sentinel (or the history it held).  The hd-64 and hd-128 widths
are also built in f32 (row paths and continuation against an f32-rounding bound, where the mask and position checks are sharp).  Row counts
B x T pick llm_forward_impl's paths (prefill_ref.path_of): 20 skinny with the fused SwiGLU, 57 skinny, 300 row-major, 650 ping-pong or
row-major (N % 256), 1100 ping-pong (256 x 256 with GEMM_PP 0) with one sequence over 9 query tiles."""
import pytest
import torch

from tests import prefill_ref as P
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TEXT_VOCAB = 4096
SENTINEL = 0x4B3D            # bf16 12 160
SHAPES = [(512, 4096, 8, 2), (1024, 4096, 8, 1), (1536, 8704, 12, 2), (2048, 5632, 32, 4), (4096, 4096, 64, 32), (1536, 8960, 12, 2),
          (896, 4864, 14, 2)]
CASES = [(1, 20), (3, 19), (2, 150), (5, 130), (1, 1100)]
CHUNKS = [(0, 37), (37, 150), (187, 13)]                 # (pos0, rows): off-tile q_pos0, a 128-row tile crossed, a skinny tail
POSITIONS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 517, 1000]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")


def _opt(name, value):
    from audio_intelligence_amd import _lib as L
    L.check(L.lib().afhip_set_option(name.encode(), int(value)))


@pytest.fixture(autouse=True)
def _defaults():
    yield
    if torch.cuda.is_available():
        for name in ("GEMM_PP", "DECODE_LEAN"):
            _opt(name, 1)
        _opt("DECODE_MERGE", 0)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "H%d_I%d_q%d_kv%d" % s)
def wide(request):
    _need_gpu()
    torch.set_num_threads(H.cpu_threads())
    model, sd, cfg = H.build_llm_at(request.param, TEXT_VOCAB)
    state = {"bf16": sd, "refs": {}}
    yield request.param, model, state, cfg
    del model, state
    torch.cuda.empty_cache()


def _ids(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, TEXT_VOCAB, (B, T), generator=g)


def _ref(state, key, fn):
    if key not in state["refs"]:
        state["refs"][key] = fn()
    return state["refs"][key]


def _cache(model, Bc, cap):
    c = model.new_cache(Bc, cap)
    for t in (c.k, c.v):
        t.view(torch.int16).fill_(SENTINEL)
    return c


def _check(tag, run_k, run_v, hid, ref, Hd, p8=False, f32=False):
    """run_k / run_v [L, B, n_kv, T, hd] device rows, hid [B, T, H]: every row within prefill_ref's bounds (f32: in f32 ulps)"""
    run = P.SimpleNamespace(k=run_k.cpu().to(torch.float64), v=run_v.cpu().to(torch.float64), hidden=hid.cpu().to(torch.float64))
    assert bool(torch.isfinite(run.k).all() and torch.isfinite(run.v).all() and torch.isfinite(run.hidden).all()), tag
    errs = P.row_errors(run, ref, f32)
    print(f"{tag}: " + ", ".join(f"{n}{'' if l is None else l} {float(mx.max()):.2f}/{float(mn.max()):.3f}" for (n, l), (mx, mn) in errs.items()))
    for (name, l), (mx, mn) in errs.items():
        bmx, bmn = P.row_bounds("hidden" if l is None else "kv", l, Hd, p8, rows=run.hidden.shape[1], f32=f32)
        bad = ((mx > bmx) | (mn > bmn)).nonzero().tolist()
        assert not bad, f"{tag}: {name} layer {l} rows (b, t) {bad[:8]} break {(bmx, bmn)}: max {float(mx.max()):.2f} mean {float(mn.max()):.3f}"


def _prefill(model, x, pos0, cache, B):
    """afhip_llm_forward of x [B, T, H] at pos0 into `cache` (batch >= B)"""
    T = x.shape[1]
    pk = model.pack(cache.cap)
    ws = model._workspace(B, T, cache.cap)
    hid = torch.ops.afhip.llm_forward(pk.blob, x.contiguous(), pos0, cache.k[:, :], cache.v[:, :], ws)
    torch.cuda.synchronize()
    return hid


def _untouched(cache, before, B, lo, hi):
    """no cache row outside [lo, hi) of the first B sequences changed"""
    for got, was in zip((cache.k, cache.v), before):
        g16, w16 = got.view(torch.int16), was.view(torch.int16)
        assert torch.equal(g16[:, :, :, :lo], w16[:, :, :, :lo]), "rows before pos0 changed"
        assert torch.equal(g16[:, :, :, hi:], w16[:, :, :, hi:]), "rows past pos0 + T changed"
        assert torch.equal(g16[:, B:], w16[:, B:]), "sequences past the batch changed"


def _path(shape, rows, T, fp8_prefill=False, w8=False):
    Hd, I, nq, nkv = shape
    hd = Hd // nq
    return P.path_of(rows, T, Hd, I, (nq + 2 * nkv) * hd, nq * hd, fp8_prefill, w8)


def _run_case(shape, model, state, cfg, B, T, tag="", w8=False):
    Hd = shape[0]
    sd = state["bf16"]
    ids = _ids(B, T, seed=B * 1000 + T)
    ref = _ref(state, ("bf16", B, T), lambda: P.forward(sd, cfg, sd["model.embed_tokens.weight"][ids], 0, None, None))
    model.enable_fp8_decode(w8)
    x = model.model.embed_tokens.weight[ids.to(DEV)]
    cache = _cache(model, B + 2, T + 40)
    before = (cache.k.clone(), cache.v.clone())
    hid = _prefill(model, x, 0, cache, B)
    path = _path(shape, B * T, T)
    _check(f"{shape} B{B} T{T} {path}{tag}", cache.k[:, :B, :, :T], cache.v[:, :B, :, :T], hid, ref, Hd)
    _untouched(cache, before, B, 0, T)
    return cache.k[:, :B, :, :T].clone(), hid


@pytest.mark.parametrize("B,T", CASES, ids=lambda v: str(v))
def test_prefill_rows_match_f64(wide, B, T):
    """each row-count path in bf16 (and 1100 rows once more with GEMM_PP 0): K/V rows and hidden rows within the bounds, the rest of the
    cache untouched; W8A16 decode weights on, the skinny and row-major prefill gives the same bits (prefill keeps the bf16 weights)"""
    shape, model, state, cfg = wide
    k, hid = _run_case(shape, model, state, cfg, B, T)
    if T == 1100:
        _opt("GEMM_PP", 0)
        _run_case(shape, model, state, cfg, B, T, tag=" GEMM_PP 0")
        _opt("GEMM_PP", 1)
    if B * T <= 300:
        k8, hid8 = _run_case(shape, model, state, cfg, B, T, tag=" W8A16 on", w8=True)
        model.enable_fp8_decode(False)
        assert torch.equal(k8.view(torch.int16), k.view(torch.int16)) and torch.equal(hid8.view(torch.int16), hid.view(torch.int16)), \
            f"{shape} B{B} T{T}: prefill changed with the e4m3 decode copies on"


def test_prefill_continuation_chunks(wide):
    """one 200-row prompt as chunks of 37 / 150 / 13 rows at pos0 0 / 37 / 187 through one cache: each chunk's rows against the one-shot
    reference's rows, nothing outside the chunk's rows changed"""
    shape, model, state, cfg = wide
    sd = state["bf16"]
    model.enable_fp8_decode(False)
    ids = _ids(1, 200, seed=77)
    ref = _ref(state, ("bf16", "prompt200"), lambda: P.forward(sd, cfg, sd["model.embed_tokens.weight"][ids], 0, None, None))
    x = model.model.embed_tokens.weight[ids.to(DEV)]
    cache = _cache(model, 3, 240)
    for pos0, n in CHUNKS:
        before = (cache.k.clone(), cache.v.clone())
        hid = _prefill(model, x[:, pos0:pos0 + n], pos0, cache, 1)
        _check(f"{shape} chunk pos0 {pos0} T{n} {_path(shape, n, n)}", cache.k[:, :1, :, pos0:pos0 + n], cache.v[:, :1, :, pos0:pos0 + n], hid,
               P.slice_rows(ref, pos0, pos0 + n), shape[0])
        _untouched(cache, before, 1, pos0, pos0 + n)


@pytest.mark.parametrize("B,T", [(5, 130), (1, 1100)], ids=lambda v: str(v))
def test_prefill_e4m3(wide, B, T):
    """enable_fp8(): e4m3 x e4m3 projections against the reference on the device-quantised weights with the e4m3 activation rounding, and
    not the bits of the bf16 prefill (the e4m3 path really ran); at H 896 (H % 256 != 0) the prefill falls back to the bf16 path: the same
    bits as with fp8 off"""
    shape, model, state, cfg = wide
    Hd = shape[0]
    ids = _ids(B, T, seed=B * 1000 + T)
    x = model.model.embed_tokens.weight[ids.to(DEV)]
    path = _path(shape, B * T, T, fp8_prefill=True)
    model.enable_fp8(True)
    try:
        cache = _cache(model, B + 2, T + 40)
        before = (cache.k.clone(), cache.v.clone())
        hid = _prefill(model, x, 0, cache, B)
        _untouched(cache, before, B, 0, T)
        k8, v8 = cache.k[:, :B, :, :T].clone(), cache.v[:, :B, :, :T].clone()
    finally:
        model.enable_fp8(False)
    cache = _cache(model, B + 2, T + 40)
    hid16 = _prefill(model, x, 0, cache, B)
    same = torch.equal(hid16.view(torch.int16), hid.view(torch.int16)) and torch.equal(cache.k[:, :B, :, :T].view(torch.int16), k8.view(torch.int16))
    if path != "p8":
        assert Hd % 256 != 0
        assert same, f"{shape} B{B} T{T}: enable_fp8 changed a prefill that must fall back to bf16"
        print(f"{shape} B{B} T{T} enable_fp8: bf16 fallback, bit-identical")
        return
    assert not same, f"{shape} B{B} T{T}: enable_fp8 gave the bf16 prefill's bits: the e4m3 path did not run"
    changed = float((hid16.float() != hid.float()).float().mean())
    assert changed > 0.5, f"{shape} B{B} T{T}: only {changed:.1%} of the hidden values differ from the bf16 prefill"
    if "w8" not in state:
        state["w8"] = P.dequantize_e4m3(state["bf16"], device=DEV)[0]
    sd8 = state["w8"]
    ref = _ref(state, ("p8", B, T), lambda: P.forward(sd8, cfg, state["bf16"]["model.embed_tokens.weight"][ids], 0, None, None, hook=P.e4m3_activations))
    _check(f"{shape} B{B} T{T} p8", k8, v8, hid, ref, Hd, p8=True)


def test_one_token_forward_w8a16(wide):
    """T = 1 afhip_llm_forward with the e4m3 decode copies (the one-token form of inference_segment): against the dequantised reference"""
    shape, model, state, cfg = wide
    B, P0 = 3, 45
    if "w8" not in state:
        state["w8"] = P.dequantize_e4m3(state["bf16"], device=DEV)[0]
    ids = _ids(B, P0 + 1, seed=5)
    sd = state["bf16"]
    emb = sd["model.embed_tokens.weight"]
    hist = _ref(state, ("bf16", "hist45"), lambda: P.forward(sd, cfg, emb[ids[:, :P0]], 0, None, None))
    model.enable_fp8_decode(True)
    try:
        cache = _cache(model, B + 2, P0 + 40)
        cache.k[:, :B, :, :P0] = hist.k.to(cache.k.dtype).to(DEV)
        cache.v[:, :B, :, :P0] = hist.v.to(cache.v.dtype).to(DEV)
        before = (cache.k.clone(), cache.v.clone())
        ref = P.forward(state["w8"], cfg, emb[ids[:, P0:]], P0, hist.k, hist.v)
        hid = _prefill(model, model.model.embed_tokens.weight[ids[:, P0:].to(DEV)], P0, cache, B)
        _check(f"{shape} T1 B{B} w8a16", cache.k[:, :B, :, P0:P0 + 1], cache.v[:, :B, :, P0:P0 + 1], hid, ref, shape[0])
        _untouched(cache, before, B, P0, P0 + 1)
    finally:
        model.enable_fp8_decode(False)


RAGGED = [(1, "w8a16", 0), (5, "w8a16", 0), (16, "w8a16", 700), (33, "bf16", 0), (70, "bf16", 700), (5, "bf16", 0)]


@pytest.mark.parametrize("B,mode,extra", RAGGED, ids=lambda v: str(v))
def test_ragged_forward(wide, B, mode, extra):
    """afhip_llm_forward_ragged: per-sequence positions from POSITIONS, the history's last key and the first key of its last 128-key range
    holding most of the softmax weight (so a range cut a key short or a dropped range breaks the bounds), the sentinel past each
    sequence's position, max_pos = the largest position (+ `extra`); the appended row at seq_pos[b] and the hidden row within the bounds, no other cache row changed.  At the hd-128
    width the B = 5 bf16 case runs again with DECODE_MERGE 1 and with DECODE_LEAN 0."""
    shape, model, state, cfg = wide
    Hd, I, nq, nkv = shape
    hd = Hd // nq
    g = torch.Generator().manual_seed(B * 7 + extra)
    sp = torch.tensor([POSITIONS[(3 * b + B) % len(POSITIONS)] for b in range(B)])
    max_pos = int(sp.max()) + extra
    if mode == "w8a16" and "w8" not in state:
        state["w8"] = P.dequantize_e4m3(state["bf16"], device=DEV)[0]
    sd = state["w8"] if mode == "w8a16" else state["bf16"]
    P_ = int(sp.max())
    kh = (torch.randn(2, B, nkv, max(P_, 1), hd, generator=g) * 0.06 * Hd ** 0.5).to(torch.bfloat16)
    vh = (torch.randn(2, B, nkv, max(P_, 1), hd, generator=g) * 0.02 * Hd ** 0.5).to(torch.bfloat16)
    ids = _ids(B, 1, seed=B + extra)
    x_ref = state["bf16"]["model.embed_tokens.weight"][ids]
    kh = P.weighted_history(sd, cfg, x_ref, sp, kh, vh)           # the last history key and the last range's first key carry the weight
    ref = P.forward(sd, cfg, x_ref, 0, kh, vh, seq_pos=sp)
    variants = [("", {})]
    if hd == 128 and B == 5 and mode == "bf16":
        variants += [(" DECODE_MERGE 1", {"DECODE_MERGE": 1}), (" DECODE_LEAN 0", {"DECODE_LEAN": 0})]
    model.enable_fp8_decode(mode == "w8a16")
    try:
        for tag, opts in variants:
            for k_, v_ in opts.items():
                _opt(k_, v_)
            cache = _cache(model, B + 2, max_pos + 1)
            for b in range(B):
                n = int(sp[b])
                cache.k[:, b, :, :n] = kh[:, b, :, :n].to(DEV)
                cache.v[:, b, :, :n] = vh[:, b, :, :n].to(DEV)
            before = (cache.k.clone(), cache.v.clone())
            pk = model.pack(cache.cap)
            ws = model._workspace(B, 1, cache.cap)
            x = model.model.embed_tokens.weight[ids[:, 0].to(DEV)].contiguous()
            hid = torch.ops.afhip.llm_forward_ragged(pk.blob, x, sp.to(device=DEV, dtype=torch.int32), max_pos, cache.k, cache.v, ws)
            torch.cuda.synchronize()
            rk = torch.stack([cache.k[:, b, :, int(sp[b])] for b in range(B)], 1)[:, :, :, None]
            rv = torch.stack([cache.v[:, b, :, int(sp[b])] for b in range(B)], 1)[:, :, :, None]
            _check(f"{shape} ragged B{B} {mode} max_pos {max_pos}{tag}", rk, rv, hid[:, None], ref, Hd)
            for got, was in zip((cache.k, cache.v), before):
                g16, w16 = got.view(torch.int16).clone(), was.view(torch.int16)
                for b in range(B):
                    g16[:, b, :, int(sp[b])] = w16[:, b, :, int(sp[b])]
                assert torch.equal(g16, w16), f"{shape} ragged B{B}{tag}: a cache row other than seq_pos[b] changed"
            for k_ in opts:
                _opt(k_, 1 if k_ != "DECODE_MERGE" else 0)
    finally:
        model.enable_fp8_decode(False)


# ---- f32 models: the f32 GEMM / skinny / attention kernels, bound = f32 rounding (prefill_ref.F32_BOUNDS, e in f32 ulps) ----------------

F32_SHAPES = [(512, 4096, 8, 2), (1024, 4096, 8, 1)]


@pytest.fixture(scope="module", params=F32_SHAPES, ids=lambda s: "f32_H%d_I%d_q%d_kv%d" % s)
def wide32(request):
    _need_gpu()
    torch.set_num_threads(H.cpu_threads())
    model, sd, cfg = H.build_llm_at(request.param, TEXT_VOCAB, dtype=torch.float32)
    state = {"f32": sd, "refs": {}}
    yield request.param, model, state, cfg
    del model, state
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B,T", CASES, ids=lambda v: str(v))
def test_f32_prefill_rows_match_f64(wide32, B, T):
    """f32 model, each row-count path (1100 rows also with GEMM_PP 0): K/V and hidden rows within the f32 bounds, the rest of the cache
    untouched"""
    shape, model, state, cfg = wide32
    sd = state["f32"]
    ids = _ids(B, T, seed=B * 1000 + T)
    ref = _ref(state, (B, T), lambda: P.forward(sd, cfg, sd["model.embed_tokens.weight"][ids], 0, None, None, store=P.f32))
    x = model.model.embed_tokens.weight[ids.to(DEV)]
    for pp in ((1, 0) if T == 1100 else (1,)):
        _opt("GEMM_PP", pp)
        cache = _cache(model, B + 2, T + 40)
        before = (cache.k.clone(), cache.v.clone())
        hid = _prefill(model, x, 0, cache, B)
        _check(f"{shape} f32 B{B} T{T} {_path(shape, B * T, T)}{'' if pp else ' GEMM_PP 0'}", cache.k[:, :B, :, :T], cache.v[:, :B, :, :T], hid,
               ref, shape[0], f32=True)
        _untouched(cache, before, B, 0, T)
    _opt("GEMM_PP", 1)


def test_f32_prefill_continuation_chunks(wide32):
    """f32 model: the 200-row prompt as chunks of 37 / 150 / 13 rows at pos0 0 / 37 / 187, each against the one-shot reference"""
    shape, model, state, cfg = wide32
    sd = state["f32"]
    ids = _ids(1, 200, seed=77)
    ref = _ref(state, "prompt200", lambda: P.forward(sd, cfg, sd["model.embed_tokens.weight"][ids], 0, None, None, store=P.f32))
    x = model.model.embed_tokens.weight[ids.to(DEV)]
    cache = _cache(model, 3, 240)
    for pos0, n in CHUNKS:
        before = (cache.k.clone(), cache.v.clone())
        hid = _prefill(model, x[:, pos0:pos0 + n], pos0, cache, 1)
        _check(f"{shape} f32 chunk pos0 {pos0} T{n}", cache.k[:, :1, :, pos0:pos0 + n], cache.v[:, :1, :, pos0:pos0 + n], hid,
               P.slice_rows(ref, pos0, pos0 + n), shape[0], f32=True)
        _untouched(cache, before, 1, pos0, pos0 + n)
