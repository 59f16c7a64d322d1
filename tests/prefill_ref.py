"""Float64 restatement of the multi-token Qwen2 forward -- what `afhip_llm_forward` (T >= 1, any pos0) and `afhip_llm_forward_ragged`
(T = 1, one position per sequence) compute (test infrastructure).

Per sequence b and query row t at position p = pos0 + t (ragged: seq_pos[b]): per layer RMSNorm, q / k / v with bias, RoPE at p, GQA
attention over the sequence's K/V history rows [0, p0_b) and the new rows up to p (causal), o, residual, post-norm, SwiGLU MLP, down,
residual (modeling_qwen2.py:35-49,91-136,150-173,195-299); the final norm.  The input is the [B, T, H] embedding rows, the output the
appended K/V rows of every layer (K after RoPE) and the final-normed hidden [B, T, H].

Rounding: float64 everywhere, except where the model STORES a tensor in bf16 (`round_bf16=True`): the residual stream after each add and
the appended K/V rows -- as tests/decode_ref.py, whose bf16 / ulp / RoPE-table helpers this file shares.

Where the HIP forward rounds internally (read from the kernels; NOT mirrored by default -- the tests emulate them through `hook`):
  unfused norm (rmsnorm_kernel, norm.hip:127): bf16(gain * bf16(x * r)), r = rsqrt(mean x^2 + eps) -- every norm of the row-major and
      ping-pong paths, and the final norm of every path                                                sites "xr", "normed"
  folded norm (skinny GEMM A-load, gemm_skinny.hip:132-148,295,315): the A operand is bf16(x * gain), the row scale r multiplies the f32
      accumulator in the epilogue -- q|k|v and gate/up of the skinny path (rows <= 64); forward(folded=True)   site "act"
  q|k|v after bias, bf16 (GEMM epilogue)                                                               site "qkv"
  q after RoPE, bf16 (rope_kv_kernel, norm.hip:171; the decode attention rotates q into a bf16 fragment too); K after RoPE is stored
      in bf16 anyway                                                                                    site "q_rope"
  the attention output, bf16                                                                           site "att"
  gate / up, bf16 (skinny 33..64 rows: stored, then swiglu_interleaved_kernel)                         site "gu"
  the SwiGLU output, bf16                                                                              site "swiglu"
  e4m3 prefill (p8): the A operand of each projection is quantised per row by afhip_quant_rows: qkv / gu from the f32 unfused norm
      gain * bf16(x * r) (mode 2, NOT rounded to bf16), o / down from the bf16 attention / SwiGLU output (mode 0); scale amax / 448,
      q = e4m3(a / scale); `e4m3_rows` below                                     sites "a_qkv", "a_o", "a_gu", "a_down"
plus f32 accumulation everywhere.  `hook(site, layer, tensor) -> tensor` is called at these sites and at the fault sites below; the
default hook is the identity.  Norm sites use decode_ref's layer numbering: l = input norm, l + 0.5 = post-attention norm, L = final.
  "w_qkv" / "w_o" / "w_gu" / "w_down"   the float64 weight a projection multiplies with ([N, K]; w_gu = gate rows, then up)
  "gain" / "rms"   a norm gain / the per-row scale [B, T] of that norm
  "bias"           the q|k|v bias
  "positions"      [B, T] the RoPE positions (int64)
  "history"        [B] the number of history rows each sequence attends (int64)
  "kv_map"         [n_q] the kv head of each query head
  "mask"           [B, T, Tk] bool, key visible to the query row (keys = history rows, then the new rows; Tk padded across b)
  "scores"         [B, n_q, T, Tk] the pre-softmax scores, masked keys at -inf
"""
from types import SimpleNamespace

import torch

from tests.decode_ref import F64, bf16, ulp_bf16, rope_tables, dequantize_e4m3, kv_error, _rot_half, _ident  # noqa: F401


def f32(t):
    """round to f32 (nearest even), returned as float64"""
    return t.to(torch.float32).to(F64)


def ulp_f32(t):
    """f32 ulp of |t| (2^-149 floor)"""
    a = t.abs().to(F64).clamp_min(2.0 ** -126)
    return torch.ldexp(torch.ones_like(a), torch.frexp(a)[1] - 24)


def e4m3_rows(a):
    """afhip_quant_rows on a [..., K] activation: per row scale = f32(amax / 448) (1 for an all-zero row), q = e4m3(a / scale) (nearest
    even); returns the dequantised q * scale in float64"""
    a = a.to(F64)
    am = a.abs().amax(-1, keepdim=True).to(torch.float32)
    sc = torch.where(am > 0, am / 448.0, torch.ones_like(am)).to(F64)
    q = (a / sc).to(torch.float32).to(torch.float8_e4m3fn).to(F64)
    return q * sc


def forward(sd, cfg, x, pos0, k_hist, v_hist, seq_pos=None, round_bf16=True, hook=None, folded=False, store=None):
    """The forward of B sequences of T new rows each.
    sd: HF-named weights (any float dtype, used as float64); cfg as decode_ref.decode_step.  x [B, T, H] the embedding rows.
    pos0: the position of row 0 of every sequence, or seq_pos [B] (T = 1): sequence b's one row sits at seq_pos[b].
    k_hist / v_hist [L, >= B, n_kv, >= history, hd] (or None with no history): rows [0, pos0) (ragged: [0, seq_pos[b])) of sequence b.
    folded: the q|k|v and gate/up norms take the skinny GEMM's folded form (the final norm never does).
    store: the rounding of the stored tensors (residual stream, K/V rows) when not bf16 -- `f32` for an f32 model.
    Returns k, v [L, B, n_kv, T, hd] (the appended rows), hidden [B, T, H] (final-normed) and x [B, T, H] (the residual stream)."""
    hook = hook or _ident
    rnd = store or (bf16 if round_bf16 else (lambda t: t))
    w = lambda name: sd[name].to(F64)
    x = torch.as_tensor(x).to(F64)
    B, T, Hd = x.shape
    L = cfg["num_hidden_layers"]
    nq, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = cfg.get("head_dim") or Hd // nq
    I, eps = cfg["intermediate_size"], cfg["rms_norm_eps"]
    rep = nq // nkv
    if seq_pos is not None:
        assert T == 1, "seq_pos: one row per sequence"
        p0 = torch.as_tensor(seq_pos).long().cpu().reshape(B)
    else:
        p0 = torch.full((B,), int(pos0), dtype=torch.int64)
    pos = p0[:, None] + torch.arange(T)[None, :]                              # [B, T] logical positions (mask, history)
    theta = cfg.get("rope_theta", 10000.0)

    def norm(x, gain_name, layer):
        """unfused form: the normed rows (what the GEMM multiplies)"""
        g = hook("gain", layer, w(gain_name))
        rs = hook("rms", layer, torch.rsqrt(x.pow(2).mean(-1) + eps))
        return hook("normed", layer, g * hook("xr", layer, x * rs[..., None]))

    def norm_proj(x, gain_name, layer, site, a_site, W):
        W = hook(site, int(layer), W)
        if folded:
            g = hook("gain", layer, w(gain_name))
            rs = hook("rms", layer, torch.rsqrt(x.pow(2).mean(-1) + eps))
            a = hook(a_site, int(layer), hook("act", layer, x * g))
            return (a @ W.T) * rs[..., None]
        return hook(a_site, int(layer), norm(x, gain_name, layer)) @ W.T

    ks, vs = [], []
    for l in range(L):
        p = f"model.layers.{l}."
        wq = torch.cat([w(p + "self_attn.q_proj.weight"), w(p + "self_attn.k_proj.weight"), w(p + "self_attn.v_proj.weight")])
        bq = hook("bias", l, torch.cat([w(p + "self_attn.q_proj.bias"), w(p + "self_attn.k_proj.bias"), w(p + "self_attn.v_proj.bias")]))
        qkv = hook("qkv", l, norm_proj(x, p + "input_layernorm.weight", l, "w_qkv", "a_qkv", wq) + bq)
        q = qkv[..., : nq * hd].reshape(B, T, nq, hd)
        k = qkv[..., nq * hd: (nq + nkv) * hd].reshape(B, T, nkv, hd)
        v = qkv[..., (nq + nkv) * hd:].reshape(B, T, nkv, hd)
        rp = hook("positions", l, pos.clone())
        cos, sin = rope_tables(rp.reshape(-1), hd, theta)
        cos, sin = cos.view(B, T, 1, hd), sin.view(B, T, 1, hd)
        q = hook("q_rope", l, q * cos + _rot_half(q) * sin)
        k = rnd(k * cos + _rot_half(k) * sin)
        v = rnd(v)
        ks.append(k.permute(0, 2, 1, 3))
        vs.append(v.permute(0, 2, 1, 3))
        # keys: history rows [0, n_hist[b]) then the T new rows; padded to a common Tk across b with invisible keys
        n_hist = hook("history", l, p0.clone())
        Tk = int(n_hist.max()) + T
        kk = torch.zeros(B, Tk, nkv, hd, dtype=F64)
        vv = torch.zeros(B, Tk, nkv, hd, dtype=F64)
        kpos = torch.full((B, Tk), 2 ** 62, dtype=torch.int64)
        for b in range(B):
            n = int(n_hist[b])
            if n:
                kk[b, :n] = k_hist[l, b, :, :n].to(F64).permute(1, 0, 2)
                vv[b, :n] = v_hist[l, b, :, :n].to(F64).permute(1, 0, 2)
                kpos[b, :n] = torch.arange(n)
            kk[b, n:n + T], vv[b, n:n + T], kpos[b, n:n + T] = k[b], v[b], pos[b]
        mask = hook("mask", l, kpos[:, None, :] <= pos[:, :, None])                 # [B, T, Tk]
        kv_map = hook("kv_map", l, torch.arange(nq) // rep)
        kq, vq = kk[:, :, kv_map], vv[:, :, kv_map]                                 # [B, Tk, nq, hd]
        s = torch.einsum("bthd,bshd->bhts", q, kq) * hd ** -0.5
        s = hook("scores", l, s.masked_fill(~mask[:, None], float("-inf")))
        att = torch.einsum("bhts,bshd->bthd", torch.softmax(s, dim=-1), vq).reshape(B, T, nq * hd)
        att = hook("att", l, att)
        x = rnd(x + hook("a_o", l, att) @ hook("w_o", l, w(p + "self_attn.o_proj.weight")).T)
        wgu = torch.cat([w(p + "mlp.gate_proj.weight"), w(p + "mlp.up_proj.weight")])
        gu = hook("gu", l, norm_proj(x, p + "post_attention_layernorm.weight", l + 0.5, "w_gu", "a_gu", wgu))
        act = hook("swiglu", l, torch.nn.functional.silu(gu[..., :I]) * gu[..., I:])
        x = rnd(x + hook("a_down", l, act) @ hook("w_down", l, w(p + "mlp.down_proj.weight")).T)

    hidden = norm(x, "model.norm.weight", L)
    return SimpleNamespace(k=torch.stack(ks), v=torch.stack(vs), hidden=hidden, x=x)


# ---- emulation of each HIP path's internal roundings (the sites above) -------------------------------------------------------------------

def path_of(rows, T, hidden, inter, qw, nqhd, fp8_prefill=False, w8_decode=False):
    """the path llm_forward_impl (csrc/llm.hip) takes for the projections of a forward over `rows` = B * T rows:
    "skinny-fused" (rows <= 32, RMSNorm folded, SwiGLU in the gate/up epilogue), "skinny" (33..64: gate/up stored, then SwiGLU),
    "w8a16" (T = 1, rows <= 32 on the e4m3 copies), "p8" (e4m3 prefill), "rowmajor" / "pingpong" (unfused norm; which GEMM kernel
    runs the projections: pingpong when rows >= 512 and every N % 256 == 0 -- informational, the roundings are the same)"""
    if rows <= 64:
        if w8_decode and T == 1 and rows <= 32:
            return "w8a16"
        return "skinny-fused" if rows <= 32 and 2 * inter >= 8192 else "skinny"
    if fp8_prefill and hidden % 256 == 0 and inter % 256 == 0 and nqhd % 256 == 0 and qw % 256 == 0 and inter <= 20480:
        return "p8"
    ns = (qw, hidden, 2 * inter)
    return "pingpong" if rows >= 512 and all(n % 256 == 0 for n in ns) else "rowmajor"


def emulate(path, n_layers):
    """hook emulating the internal bf16 (and e4m3) roundings of `path` (path_of) in a model of `n_layers` layers; run the reference
    with folded=is_folded(path)"""
    sites = {"xr", "normed", "act", "qkv", "q_rope", "att", "swiglu"} | ({"gu"} if path == "skinny" else set())

    def hook(site, layer, t):
        if path == "p8":
            if site == "normed" and layer != n_layers:      # quant_rows mode 2: gain * bf16(x * r) stays f32 before the e4m3 step
                return t
            if site in ("a_qkv", "a_o", "a_gu", "a_down"):
                return e4m3_rows(t)
        return bf16(t) if site in sites else t
    return hook


def emulate_f32(site, layer, t):
    """the internal roundings of an f32 model: the same sites as emulate(), every one an f32 store (run with store=f32)"""
    return f32(t) if site in ("xr", "normed", "act", "qkv", "q_rope", "att", "gu", "swiglu") else t


def e4m3_activations(site, layer, t):
    """the reference hook of the e4m3 prefill: the activations quantised as afhip_quant_rows does, everything else float64"""
    return e4m3_rows(t) if site in ("a_qkv", "a_o", "a_gu", "a_down") else t


def is_folded(path):
    return path in ("skinny", "skinny-fused", "w8a16")


# ---- tolerances of the GPU checks (tests/test_gpu_prefill_widths.py) ---------------------------------------------------------------------
#
# Per appended K/V row and per hidden row: decode_ref's normalised error e = |hip - ref| / (ulp(|ref|) + ulp(rms / 4)), rms = that
# row's root mean square (all kv heads), as max / mean over the row.  See row_bounds.


def row_error(hip, ref):
    """[..., R, n_kv, hd] K/V rows or [..., R, H] hidden rows (add a unit axis) -> (max e, mean e) per leading index"""
    return kv_error(hip, ref)
#
# Bounds, set by the emulated rounding points above (test_prefill_ref_host prints them per width, path and layer; measured here at 187
# rows, max / mean of the row means: layer 0 <= 12.9 / 0.88, layer 1 K/V 8.6 / 1.06 at H 512 up to 74 / 6.1 at H 4096, hidden 5.7 / 0.69
# at H 512 up to 221 / 15.5 at H 4096; e4m3 prefill against the e4m3-activation reference: layer 0 59 / 4.2, layer 1 up to 348 / 26,
# hidden up to 1000 / 67).  On the MI355X (tests/test_gpu_prefill_widths.py) the worst rows were: layer 0 10.4 / 0.86; layer 1 K/V
# 10.6 / 1.08 at H 512 up to 107 / 8.3 at H 4096 (1100 rows); hidden 330 / 27 at H 4096 (1100 rows); e4m3 prefill layer 1 431 / 31 and
# hidden 1019 / 78 at H 4096:
#   layer 0 K/V   as decode_ref's layer 0 (R1 + the q|k|v rounding + the RoPE rounding of K), the maximum taken over every row of a prefill
#   layer 1 K/V and the hidden rows   layer 0's roundings reach them through the sharp softmax of these weights and two residual adds (the
#                 final norm divides by a row rms that the MLP has shrunk), growing with the width
#   p8            the device's activation lands on a neighbouring e4m3 value (1/16 relative) wherever its bf16 difference from the
#                 reference straddles an e4m3 rounding boundary, so every layer sits near the bf16 path's layer-1 scale, and above it


def row_bounds(kind, layer, hidden, p8=False, rows=128, f32=False):
    """(max e, mean e) allowed for one appended K/V row of `layer` (kind "kv") or one final hidden row (kind "hidden") in a forward of
    `rows` rows per sequence: past layer 0 the bound grows by rows / 4096 (the tail of more rows; measured on the MI355X at H 4096:
    layer-1 K mean 6.6 at 150 rows, 8.3 at 1100).  f32: e in f32 ulps (row_errors(f32=True)); see F32_BOUNDS."""
    grow = 1.0 + rows / 4096
    if f32:
        mx, mn = F32_BOUNDS["hidden" if kind == "hidden" else min(layer, 1)]
        return (mx * grow, mn * grow)
    if kind == "hidden":
        mx, mn = (200.0 + hidden / 3, 20.0 + hidden / 64) if p8 else (30.0 + hidden / 12, 2.0 + hidden / 192)
        return (mx * grow, mn * grow)
    if layer == 0:
        return (100.0, 8.0) if p8 else (16.0, 1.2)
    mx, mn = (60.0 + hidden / 8, 8.0 + hidden / 128) if p8 else (12.0 + hidden / 48, 1.0 + hidden / 640)
    return (mx * grow, mn * grow)


# f32 models (H 512 and 1024 in the GPU test): e counted in f32 ulps.  The f32 emulation of the rounding points gives layer-0 e up to
# 7 / 0.75 and layer 1 / hidden up to 20 / 1.6; the MI355X measures more (its f32 MFMA accumulation, rsqrtf and __expf are not the f64
# sum rounded once): layer 0 up to 131 / 9.0, layer 1 K/V 180 / 17.9 and hidden 317 / 22.5 (row-major and ping-pong, H 1024).  Bounds: layer 0
# (256, 16), layer 1 and hidden (1024, 64), a relative error of ~8e-6: the f32 faults of test_prefill_ref_host (a mask off by one, the
# tile-edge row, ...) break them on every row whose attention output they move by 0.1 %.
F32_BOUNDS = {0: (256.0, 16.0), 1: (1024.0, 64.0), "hidden": (1024.0, 64.0)}


def _row_e(hip, ref, ulp):
    """decode_ref.kv_error with the ulp of `ulp`: (max e, mean e) over the last two axes"""
    hip, ref = hip.to(F64), ref.to(F64)
    rms = ref.pow(2).mean(dim=(-2, -1), keepdim=True).sqrt()
    e = (hip - ref).abs() / (ulp(ref) + ulp(rms / 4))
    return e.amax(dim=(-2, -1)), e.mean(dim=(-2, -1))


def row_errors(run, ref, f32=False):
    """per row errors of a forward against the reference: {("K" | "V", layer): (max e, mean e) [B, T]} and ("hidden", None); e in bf16
    ulps (decode_ref.kv_error), or in f32 ulps with f32=True"""
    ulp = ulp_f32 if f32 else ulp_bf16
    out = {}
    for name in ("k", "v"):
        mx, mn = _row_e(getattr(run, name).permute(0, 1, 3, 2, 4), getattr(ref, name).permute(0, 1, 3, 2, 4), ulp)   # [L, B, T]
        for l in range(mx.shape[0]):
            out[(name.upper(), l)] = (mx[l], mn[l])
    out[("hidden", None)] = _row_e(run.hidden.unsqueeze(-2), ref.hidden.unsqueeze(-2), ulp)
    return out


def rows_broken(run, ref, hidden, p8=False, f32=False):
    """[B, T] bool: some appended K/V row of that (sequence, row) or its hidden row breaks its bound"""
    bad = None
    for (name, l), (mx, mn) in row_errors(run, ref, f32).items():
        bmx, bmn = row_bounds("hidden" if l is None else "kv", l, hidden, p8, rows=run.hidden.shape[1], f32=f32)
        b = (mx > bmx) | (mn > bmn)
        bad = b if bad is None else bad | b
    return bad


def weighted_history(sd, cfg, x, seq_pos, k_hist, v_hist, margin=4.0, split=128):
    """k_hist [L, >= B, n_kv, >= max seq_pos, hd] with, for every sequence b with seq_pos[b] = n > 0, the K rows at n - 1 (the last history
    key) and at split * (n // split) (the first key of the last split-context range, when it is history) replaced per kv group by the
    direction of the group's mean query, scaled so that its score sits `margin` above the group's largest history score.  These keys then
    hold most of the softmax weight: a key range that stops a key short, or a combine that drops the last range, moves the attention output
    by a whole V row.  Built layer by layer (layer l's query depends on layer l - 1's attention) from this reference's own queries; the
    result is rounded to k_hist's dtype."""
    kh = k_hist.clone()
    nq, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = cfg.get("head_dim") or cfg["hidden_size"] // nq
    rep = nq // nkv
    sp = torch.as_tensor(seq_pos).long().cpu()
    for l in range(cfg["num_hidden_layers"]):
        got = {}

        def grab(site, layer, t):
            if site == "q_rope" and layer == l:
                got["q"] = t
            return t
        forward(sd, cfg, x, 0, kh, v_hist, seq_pos=sp, hook=grab)
        q = got["q"][:, 0]                                                   # [B, nq, hd]
        for b in range(len(sp)):
            n = int(sp[b])
            if n == 0:
                continue
            rows = sorted({n - 1, split * (n // split)} & set(range(n)))
            for g in range(nkv):
                qh = q[b, g * rep:(g + 1) * rep]
                qg = qh.mean(0)
                s_max = float((qh @ kh[l, b, g, :n].to(F64).T).max()) * hd ** -0.5
                beta = (max(s_max, 0.0) + margin) * hd ** 0.5 / float(qg.pow(2).sum())
                for r in rows:
                    kh[l, b, g, r] = (qg * beta).to(kh.dtype)
    return kh


def slice_rows(ref, t0, t1):
    """the rows [t0, t1) of a forward's result (a chunk of a one-shot reference)"""
    return SimpleNamespace(k=ref.k[:, :, :, t0:t1], v=ref.v[:, :, :, t0:t1], hidden=ref.hidden[:, t0:t1], x=ref.x[:, t0:t1])
