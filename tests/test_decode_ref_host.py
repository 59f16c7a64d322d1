"""tests/decode_ref.py on the CPU: pinned to transformers' Qwen2 in float64, and its tolerances shown to have teeth at every width of
tests/test_gpu_decode_widths.py -- the HIP step's own rounding points (emulated) stay inside them, and each planted fault breaks them for
every sequence of the batch."""
import pytest
import torch

from tests import decode_ref as R
from tests import helpers as H

F64 = torch.float64


def test_decode_ref_matches_transformers_qwen2_f64(monkeypatch):
    """A small GQA Qwen2 with biases in float64: prefill 5 tokens, decode 3 with transformers' cache; decode_ref (rounding off) on the
    same weights and the same cache gives the same new K/V rows and logits to 1e-10.  Qwen2RMSNorm and eager attention widen to f32 by
    design (modeling_qwen2.py: `.to(torch.float32)`, `softmax(..., dtype=torch.float32)`): the model runs here with SDPA attention and
    the same RMSNorm formula kept in its input dtype, so that every step is float64."""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    from transformers.models.qwen2 import modeling_qwen2 as mq

    def rms_f64(self, x):
        return self.weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.variance_epsilon))
    monkeypatch.setattr(mq.Qwen2RMSNorm, "forward", rms_f64)
    V, B = 300, 2
    hf_cfg = Qwen2Config(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                         max_position_embeddings=64, rope_theta=10000.0, rms_norm_eps=1e-6, tie_word_embeddings=False, attn_implementation="sdpa")
    g = torch.Generator().manual_seed(11)
    m = Qwen2ForCausalLM(hf_cfg).double().eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("layernorm.weight") or n == "model.norm.weight":
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g, dtype=F64))
            else:
                p.copy_((0.3 if n.endswith("bias") else 0.2) * torch.randn(p.shape, generator=g, dtype=F64))
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    cfg = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, intermediate_size=128, rope_theta=10000.0,
               rms_norm_eps=1e-6)
    ids = torch.randint(0, V, (B, 5), generator=g)
    with torch.no_grad():
        out = m(ids, use_cache=True)
        cache = out.past_key_values
        tok = out.logits[:, -1].argmax(-1)
        for step in range(3):
            T = cache.layers[0].keys.shape[2]
            kh = torch.stack([cache.layers[l].keys for l in range(2)]).clone()
            vh = torch.stack([cache.layers[l].values for l in range(2)]).clone()
            ref = R.decode_step(sd, cfg, tok, torch.full((B,), T), kh, vh, [[0, V]], round_bf16=False)
            out = m(tok[:, None], past_key_values=cache, use_cache=True)
            cache = out.past_key_values
            for l in range(2):
                assert float((cache.layers[l].keys[:, :, T] - ref.k[l]).abs().max()) <= 1e-10, (step, l)
                assert float((cache.layers[l].values[:, :, T] - ref.v[l]).abs().max()) <= 1e-10, (step, l)
            assert float((out.logits[:, -1] - ref.logits).abs().max()) <= 1e-10, step
            assert torch.equal(ref.pick, out.logits[:, -1].argmax(-1))
            tok = ref.pick


def test_decode_ref_masked_argmax_first_index_and_margin():
    """the pick is the first maximum inside the intervals; the margin is best minus second best"""
    cfg = dict(hidden_size=8, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1, intermediate_size=16, rms_norm_eps=1e-6)
    sd = {k: torch.zeros(s, dtype=F64) for k, s in H.syn.llm_param_shapes(cfg, 40, 1, 8) if not k.startswith(("adaptor", "stream"))}
    sd["model.embed_tokens.weight"] += 1.0
    sd["model.norm.weight"] += 1.0
    sd["lm_head.weight"][[5, 9, 30], 0] = 1.0                      # three tied best rows
    sd["lm_head.weight"][12, 0] = 0.5
    kh = torch.zeros(1, 1, 1, 4, 4, dtype=F64)
    r = R.decode_step(sd, cfg, [3], [0], kh, kh, [[6, 8], [9, 10], [12, 13], [30, 31]], head_rows=35)
    assert int(r.pick[0]) == 9 and float(r.margin[0]) == 0.0
    r = R.decode_step(sd, cfg, [3], [0], kh, kh, [[10, 20]], head_rows=35)
    assert int(r.pick[0]) == 12 and float(r.margin[0]) > 0
    assert r.logits.shape == (1, 35) and bool(torch.isinf(r.logits[0, :10]).all())


# ---- tolerances with teeth ----------------------------------------------------------------------------------------------------------------

SHAPES = H.LLM_WIDTHS
T0 = 37
_cfg = H.llm_cfg_at
_weights = H.llm_weights_f64


def _emulate(site, layer, t):
    """the HIP step's internal bf16 roundings R1-R5 (decode_ref's docstring)"""
    return R.bf16(t) if site in ("act", "qkv", "att", "swiglu", "logits") else t


def _distinct_tokens(sd, B, vocab):
    """B previous tokens whose embedding rows' root mean squares differ pairwise by >= 4 %: two rows with the same norm cannot tell a
    norm applied to the wrong row, and real embedding tables are far from equal-norm"""
    rms = sd["model.embed_tokens.weight"].pow(2).mean(-1).sqrt()
    order = torch.argsort(rms[1:]) + 1
    picks = [int(order[int(len(order) * f)]) for f in torch.linspace(0.02, 0.98, B).tolist()]
    r = rms[picks]
    assert float((r[1:] / r[:-1]).min()) >= 1.04
    return torch.tensor(picks)


def _faults(I, w8, scales):
    step = 128 if w8 else 64
    def drop(site, k0):
        def f(s, l, t):
            if s == site and l == 0:
                t = t.clone()
                t[:, k0:k0 + step] = 0
            return t
        return f
    def swap_rms(s, l, t):
        return t.flip(0) if s == "rms" and l == 0 else t
    def wrong_gain(sd):
        def f(s, l, t):
            return sd["model.layers.1.input_layernorm.weight"].to(F64) if s == "gain" and l == 0 else t
        return f
    def no_bias(s, l, t):
        return torch.zeros_like(t) if s == "bias" and l == 0 else t
    def swap_rows(s, l, t):
        return t.flip(0) if s == "swiglu" and l == 0 else t
    out = {"drop_qkv": drop("w_qkv", 256), "drop_o": drop("w_o", 0), "drop_gu": drop("w_gu", 384), "drop_down": drop("w_down", I - step),
           "rms_wrong_row": swap_rms, "wrong_layer_gain": wrong_gain, "no_qkv_bias": no_bias, "rows_swapped": swap_rows}
    if w8:
        def neighbour_scale(s, l, t):
            if s == "w_down" and l == 0:
                sc = scales["model.layers.0.mlp.down_proj.weight"].to(F64)
                t = t * (torch.roll(sc, -1) / sc)[:, None]
            return t
        out["e4m3_neighbour_scale"] = neighbour_scale
    return out


def _broken(run, ref, eps, hidden, w8):
    """per sequence: does `run` fail the GPU test's K/V bounds (any layer, K or V) or its pick check against `ref`?"""
    bad = R.kv_broken(run.k, ref.k, hidden, w8) | R.kv_broken(run.v, ref.v, hidden, w8)
    regret = ref.logits.max(-1).values - ref.logits.gather(1, run.pick[:, None])[:, 0]
    return bad | (regret > eps) | ((ref.margin > eps) & (run.pick != ref.pick))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d_I%d_q%d_kv%d" % s)
def test_gpu_tolerances_hold_rounding_and_catch_faults(shape):
    """At each GPU-test width, bf16 and W8A16: the reference with the HIP step's internal roundings (R1-R5) stays inside the K/V bounds and
    the pick bound; the reference with one planted fault in layer 0 (a K step of one projection dropped, the RMS scale of the other row,
    layer 1's gain, no q|k|v bias, two batch rows swapped, the e4m3 row scale of the neighbouring row) breaks them for every sequence."""
    torch.set_num_threads(H.cpu_threads())
    Hd, I, nq, nkv = shape
    cfg = _cfg(*shape)
    hd = Hd // nq
    B, vocab = 2, 2048
    sd16 = _weights(cfg, vocab)
    prev = _distinct_tokens(sd16, B, vocab)
    g = torch.Generator().manual_seed(Hd + I)
    kh = (torch.randn(2, B, nkv, T0, hd, generator=g) * 0.06 * Hd ** 0.5).to(torch.bfloat16)
    vh = (torch.randn(2, B, nkv, T0, hd, generator=g) * 0.02 * Hd ** 0.5).to(torch.bfloat16)
    iv = [[1, 2], [5, 6], [60, 70], [100, 700], [900, 1500], [1600, 2000]]
    pos = torch.full((B,), T0)
    for w8 in (False, True):
        sd, scales = R.dequantize_e4m3(sd16) if w8 else (sd16, {})
        step = lambda hook=None: R.decode_step(sd, cfg, prev, pos, kh, vh, iv, head_rows=2000, n_stream=8, hook=hook)
        ref = step()
        eps = R.pick_eps(ref.logits)
        emu = step(_emulate)
        for l in range(2):
            (kmx, kmn), (vmx, vmn) = R.kv_error(emu.k[l], ref.k[l]), R.kv_error(emu.v[l], ref.v[l])
            print(f"H{Hd} I{I} {'w8a16' if w8 else 'bf16'} layer {l}: emulated rounding e K max {float(kmx.max()):.2f} mean {float(kmn.max()):.3f}"
                  f", V max {float(vmx.max()):.2f} mean {float(vmn.max()):.3f} (bounds {R.kv_bounds(l, Hd, w8)})")
        regret = ref.logits.max(-1).values - ref.logits.gather(1, emu.pick[:, None])[:, 0]
        print(f"   pick regret {regret.tolist()} eps {eps.tolist()} margin {ref.margin.tolist()}")
        assert not bool(_broken(emu, ref, eps, Hd, w8).any())
        for name, f in _faults(I, w8, scales).items():
            f = f(sd) if name == "wrong_layer_gain" else f
            run = step(lambda s, l, t, f=f: f(s, l, _emulate(s, l, t)))
            assert bool(_broken(run, ref, eps, Hd, w8).all()), f"H{Hd} I{I} w8={w8}: fault {name} stays inside the tolerance"
