"""The AF-Whisper encoder at every width and layer form it accepts, against the float64 forward of tests/encoder_ref.py.

Each model is encoder_ref.enc_weights's recipe (2 layers, max_source_positions 1500, non-trivial LayerNorm gains / betas and biases).
Every stored state -- the stem, each layer's output judged layer-locally (the reference starts from the device's own input of that layer)
-- and the pooled output (end to end) is judged per row against encoder_ref.bounds.  Each case asserts the path afhip_encoder_path
reports.  The float64 reference runs on the GPU through torch's float64 arithmetic, which shares no code with the HIP kernels under
test (tests/test_encoder_ref_host.py pins the same function to transformers on the CPU)."""
import pytest
import torch

from tests import encoder_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
EXPLICIT = [(384, 6, 1536), (640, 10, 2560), (512, 8, 1920)]
FOLDED64 = [(512, 8, 2048), (768, 12, 3072), (1024, 16, 4096), (1280, 20, 5120)]
FOLDED128 = [(1024, 8, 4096), (1280, 10, 5120)]
SHAPES = EXPLICIT + FOLDED64 + FOLDED128
E4M3 = {(512, 8, 2048): (6, 7, 14, 15), (1280, 20, 5120): (6, 7, 14, 15), (768, 12, 3072): (6,), (1024, 8, 4096): (6,)}
KEY_LEN = [1, 65, 777, 1500]
RAGGED = [0, 63, 64, 1499, 2]
OFFSET_ROWS = {16.0: range(200, 204), 64.0: range(204, 208)}     # rows of embed_positions given a common offset of that many row stds
SPIKE_ROWS = range(208, 212)                                      # ... and one channel at +-500
# pooled rows of those stream rows: judged layer-locally and through the tail from the device's own last state, but not end to end -- one
# bf16 ulp of a stream row whose mean sits 64 stds from zero is a quarter of its std, which the final LayerNorm scales up to ~60 ulps of
# its output in the reference as on the device (measured: pooled rows 102-103 at 42-91 / 4.9-6.8 end to end at every width, the
# layer-local rows inside the bound)
SPECIAL_POOLED = range(100, 106)


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
        for name, v in (("ATTN_ENC64", 1), ("ATTN_LAG", 1), ("FP8_MASK", 6), ("FP8_FC2", 0)):
            _opt(name, v)


def _weights(cfg, dtype):
    sd = E.enc_weights(cfg)
    pos = sd["embed_positions.weight"]
    rs = float(pos.std()) * 5.0                                  # ~ a stem row's std
    for level, rows in OFFSET_ROWS.items():
        pos[list(rows)] += level * rs
    for i, r in enumerate(SPIKE_ROWS):
        pos[r, (37 * i) % cfg["d_model"]] = 500.0 if i % 2 == 0 else -500.0
    return {n: t.to(dtype) for n, t in sd.items()}


def _model(cfg, sd, dtype):
    from audio_intelligence_amd.multimodal_io.modeling_whisper import AFWhisperEncoder, AFWhisperEncoderConfig
    enc = AFWhisperEncoder(AFWhisperEncoderConfig.from_dict(cfg))
    enc.load_state_dict(sd, strict=True)
    return enc.to(DEV, dtype)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "d%d_h%d_f%d" % s)
def shape(request):
    _need_gpu()
    yield request.param
    torch.cuda.empty_cache()


def _mel(B, dtype, seed=5, max_pos=1500):
    g = torch.Generator().manual_seed(seed)
    return (0.4 * torch.randn(B, 2 * max_pos, 128, generator=g)).to(dtype)


def _sd_dev(sd):
    return {n: t.to(DEV, F64) for n, t in sd.items()}


def _w8(enc):
    """the e4m3 weights the packed model multiplies with, dequantised (the device's copy, not a CPU re-quantisation)"""
    f8 = enc.pack().f8
    out = {}
    for src in ("qkv", "out", "fc1", "fc2"):
        for l, (q8, sc) in enumerate(zip(f8[src + "_w8"], f8[src + "_s8"])):
            out[(src, l)] = q8.view(torch.float8_e4m3fn).to(F64) * sc.to(F64)[:, None]
    return out


def _form(p):
    return E.form(fold=p["folded"], mask=p["mask"] if p["e4m3"] else 0, att_static=p["att_static"], fc2_static=p["fc2_static"])


def _check(tag, got, ref, kind, d, f32_model=False, e4m3=False):
    got = got.to(F64)
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite rows"
    mx, mn = E.row_error(got, ref, f32_model)
    bmx, bmn = E.bounds(kind, d, f32_model, e4m3)
    print(f"{tag} {kind}: max {float(mx.max()):.2f} mean {float(mn.max()):.3f}  (bound {bmx:.0f} / {bmn:.2f})")
    bad = (mx > bmx) | (mn > bmn)
    assert not bool(bad.any()), f"{tag} {kind}: rows {bad.nonzero().tolist()[:8]} break the bound (max {float(mx.max()):.2f}, mean {float(mn.max()):.3f})"


def _judge(tag, enc, sd, cfg, mel, kl, f32_model=False):
    """stem, every layer (layer-locally) and the pooled output of a padded forward against the reference of the path it reports"""
    d, L = cfg["d_model"], cfg["encoder_layers"]
    p = enc.path(mel.shape[0])
    path = _form(p)
    e8 = p["e4m3"]
    kw = dict(path=path, store=E.f32 if f32_model else E.bf16, device=DEV)
    if e8:
        asc = enc._att_out_scale.tolist() if enc._att_out_scale is not None else None
        fsc = enc._fc2_in_scale.tolist() if enc._fc2_in_scale is not None else None
        kw.update(w8=_w8(enc), att_scale=asc, fc2_scale=fsc, hook=E.e4m3_hook(path, asc, fsc))
    md = mel.to(DEV)
    fl = torch.tensor(kl, dtype=torch.int32)
    klt = torch.tensor(kl)
    states = []
    for hl in range(-1, L):
        out, h = enc.encode_btc(md, feat_len=fl, hidden_layer=hl)
        states.append(h.to(F64))
    sdd = _sd_dev(sd)
    mel_bct = mel.to(DEV, F64).transpose(1, 2)
    ref_full = E.forward(sdd, cfg, mel=mel_bct, key_len=klt, **kw)
    _check(tag, states[0], ref_full.stem, "stem", d, f32_model, e8)
    for l in range(L):
        r = E.forward(sdd, cfg, x=states[l], first=l, last=l + 1, key_len=klt, **kw)
        _check(f"{tag} layer {l}", states[l + 1], r.states[0], "layer", d, f32_model, e8)
    tail = E.forward(sdd, cfg, x=states[L], first=L, key_len=klt, **kw)
    _check(f"{tag} tail", out, tail.out, "tail", d, f32_model, e8)
    keep = _plain_pooled(out.shape[1])
    _check(tag, out[:, keep], ref_full.out[:, keep], "out", d, f32_model, e8)
    return p


def _plain_pooled(n):
    return torch.tensor([r for r in range(n) if r not in SPECIAL_POOLED])


def test_encoder_widths_padded(shape, monkeypatch):
    d, nh, f = shape
    hd = d // nh
    cfg = E.enc_config(d, nh, f)
    folded = shape in FOLDED64 or shape in FOLDED128
    sd32 = _weights(cfg, torch.float32)
    enc = _model(cfg, sd32, torch.float32)
    p = _judge(f"{shape} f32", enc, sd32, cfg, _mel(len(KEY_LEN), torch.float32), KEY_LEN, f32_model=True)
    assert not p["folded"] and not p["e4m3"] and p["attention"] == "generic", p
    del enc
    sd = _weights(cfg, torch.bfloat16)
    enc = _model(cfg, sd, torch.bfloat16)
    mel = _mel(len(KEY_LEN), torch.bfloat16)
    p = _judge(f"{shape} bf16", enc, sd, cfg, mel, KEY_LEN)
    assert p["folded"] == folded and not p["e4m3"], p
    assert p["attention"] == ("enc64" if folded and hd == 64 else "generic"), p
    if folded:
        monkeypatch.setenv("AFHIP_LN_FOLD", "0")
        enc._packed = None
        try:
            p = _judge(f"{shape} bf16 LN_FOLD=0", enc, sd, cfg, mel, KEY_LEN)
            assert not p["folded"] and p["attention"] == "generic", p
        finally:
            monkeypatch.delenv("AFHIP_LN_FOLD")
            enc._packed = None
        if hd == 64:
            _opt("ATTN_ENC64", 0)
            p = _judge(f"{shape} bf16 ATTN_ENC64=0", enc, sd, cfg, mel, KEY_LEN)
            assert p["folded"] and p["attention"] == "lag", p
            _opt("ATTN_LAG", 0)
            p = _judge(f"{shape} bf16 ATTN_ENC64=0 ATTN_LAG=0", enc, sd, cfg, mel, KEY_LEN)
            assert p["folded"] and p["attention"] == "generic", p
            _opt("ATTN_ENC64", 1)
            _opt("ATTN_LAG", 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_encoder_widths_ragged(shape, dtype):
    """the packed forward's kept rows against the reference's ragged form (1 layer, so the bound is sharp), the rows behind them zero
    with a NaN-poisoned workspace"""
    d, nh, f = shape
    cfg = E.enc_config(d, nh, f, n_layers=1)
    sd = _weights(cfg, dtype)
    enc = _model(cfg, sd, dtype)
    f32_model = dtype == torch.float32
    mel = _mel(len(RAGGED), dtype, seed=6)
    p = enc.path(len(RAGGED))
    assert p["folded"] == (dtype == torch.bfloat16 and shape not in EXPLICIT), p
    ws = enc._workspace(len(RAGGED))
    ws.view(torch.int16 if dtype == torch.bfloat16 else torch.int32).fill_(-1)        # all-ones bit patterns: NaN in either dtype
    lens = torch.tensor(RAGGED, dtype=torch.int32)
    got = enc.encode_btc(mel.to(DEV), feat_len=lens, ragged=True).to(F64)
    ref = E.forward(_sd_dev(sd), cfg, mel=mel.to(DEV, F64).transpose(1, 2), lengths=RAGGED, path=_form(p),
                    store=E.f32 if f32_model else E.bf16, device=DEV)
    for b, n in enumerate(RAGGED):
        k = E.kept_rows(n)
        assert bool((got[b, k:] == 0).all()), f"{shape} clip {b} (len {n}): rows behind the kept ones must be zero"
        if k:
            keep = _plain_pooled(k)
            _check(f"{shape} {dtype} ragged clip {b} len {n}", got[b, keep], ref.out[b, keep], "out", d, f32_model)


@pytest.mark.parametrize("e4m3_shape", list(E4M3), ids=lambda s: "d%d_h%d_f%d" % s)
def test_encoder_widths_e4m3(e4m3_shape):
    _need_gpu()
    shape = e4m3_shape
    d, nh, f = shape
    cfg = E.enc_config(d, nh, f)
    sd = _weights(cfg, torch.bfloat16)
    enc = _model(cfg, sd, torch.bfloat16).enable_fp8()
    mel = _mel(len(KEY_LEN), torch.bfloat16)
    fl = torch.tensor(KEY_LEN, dtype=torch.int32)
    for mask in E4M3[shape]:
        _opt("FP8_MASK", mask & 7)
        _opt("FP8_FC2", 1 if mask & 8 else 0)
        for static in (False, True):
            if static:
                enc.calibrate_fp8(mel.to(DEV), fl)
            else:
                enc.calibrate_fp8(None)
            p = _judge(f"{shape} e4m3 mask {mask}{' static' if static else ''}", enc, sd, cfg, mel, KEY_LEN)
            assert p["e4m3"] and p["mask"] == mask and p["folded"], p
            assert p["fc2_static"] == (static and bool(mask & 4) and not mask & 8), p
            qkv_fold = not (mask & 1) and not (mask & 8)
            assert p["att_static"] == (static and bool(mask & 2) and qkv_fold and d // nh == 64), p
        enc.calibrate_fp8(None)


def test_encoder_fold_choice_depends_on_the_batch():
    """max_source_positions 250: one clip (250 rows) runs the explicit LayerNorms, three (750 rows) the folded GEMMs.  Both are within
    the bound of the same reference; they are allowed to differ in bits."""
    _need_gpu()
    cfg = E.enc_config(512, 8, 2048, max_pos=250)
    sd = _weights(cfg, torch.bfloat16)
    enc = _model(cfg, sd, torch.bfloat16)
    mel = _mel(3, torch.bfloat16, seed=8, max_pos=250)
    p1 = _judge("Tp 250 B 1", enc, sd, cfg, mel[:1], [250])
    p3 = _judge("Tp 250 B 3", enc, sd, cfg, mel, [250, 129, 64])
    assert not p1["folded"] and p3["folded"], (p1, p3)
