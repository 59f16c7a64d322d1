"""Sampled decoding through `Qwen2AudioForConditionalGeneration.generate()` (the tiny AF3 model of test_gpu_af3.py, fp32) and the UALM
route for top-k above 64: every step's processed scores and drawn token against the oracle of tests/sample_ref.py."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import sample_ref as R
from tests.test_gpu_af3 import _build, _gold, _inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gen(model, g, seed=None, **kw):
    ids, mask, feats, fmask = _inputs(g, "left")
    if seed is not None:
        kw["generator"] = torch.Generator(device=DEV).manual_seed(seed)
    return ids, model.generate(ids, input_features=feats, attention_mask=mask, feature_attention_mask=fmask, **kw)


@pytest.fixture(scope="module")
def af3():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return _build()


def test_top_k_1_sampling_is_greedy(af3):
    model, g = af3
    ids, out = _gen(model, g, seed=0, do_sample=True, top_k=1, max_new_tokens=g["n_steps"])
    assert out[:, ids.shape[1]:].cpu().tolist() == np.array(g["left"]["greedy_ids"]).T.tolist()


def test_same_seed_same_tokens(af3):
    model, g = af3
    kw = dict(do_sample=True, temperature=0.9, top_p=0.95, max_new_tokens=6)
    _, a = _gen(model, g, seed=7, **kw)
    _, b = _gen(model, g, seed=7, **kw)
    assert torch.equal(a, b)


@pytest.mark.parametrize("knobs", [dict(temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.05), dict(top_p=0.95),
                                   dict(top_k=5, temperature=1.5), dict(generation_config={"top_k": 50, "repetition_penalty": 1.2})])
def test_replay_scores_and_draws_against_the_oracle(af3, knobs):
    model, g = af3
    knobs = dict(knobs)
    n = 5
    ids, o = _gen(model, g, seed=3, do_sample=True, max_new_tokens=n, return_dict_in_generate=True, output_scores=True, output_logits=True, **knobs)
    kn = dict(knobs.pop("generation_config", {}), **knobs)
    W = ids.shape[1]
    B = ids.shape[0]
    seqs = o.sequences.cpu()
    assert len(o.scores) == len(o.logits) == seqs.shape[1] - W
    gen = torch.Generator(device=DEV).manual_seed(3)
    for s in range(len(o.scores)):
        u = torch.rand(B, generator=gen, device=DEV).cpu()
        lg, sc = o.logits[s].cpu().numpy(), o.scores[s].cpu().numpy()
        for b in range(B):
            want, keep = R.process(lg[b], penalty=kn.get("repetition_penalty", 1.0), ids=seqs[b, :W + s].numpy(),
                                   temperature=kn.get("temperature", 1.0), top_k=kn.get("top_k", 0), top_p=kn.get("top_p", 1.0))
            if kn.get("top_p", 1.0) < 1.0:
                x = R.process(lg[b], penalty=kn.get("repetition_penalty", 1.0), ids=seqs[b, :W + s].numpy(), temperature=kn.get("temperature", 1.0))[0]
                _, keep_k = R.process(lg[b], penalty=kn.get("repetition_penalty", 1.0), ids=seqs[b, :W + s].numpy(),
                                      temperature=kn.get("temperature", 1.0), top_k=kn.get("top_k", 0))
                if R.p_margin(x, keep_k, kn["top_p"]) < 1e-5:
                    continue                                   # too close to the top-p boundary for a float64 oracle
            assert np.array_equal(np.isfinite(sc[b]), keep), (s, b)
            np.testing.assert_array_equal(sc[b][keep], want[keep])
            t, dist = R.draw(want, float(u[b]))
            if dist > 1e-6:
                assert int(seqs[b, W + s]) == t, (s, b)


def test_eos_and_pad_under_sampling(af3):
    model, g = af3
    kw = dict(do_sample=True, temperature=1.3, top_k=40, max_new_tokens=6)
    ids, base = _gen(model, g, seed=11, **kw)
    W = ids.shape[1]
    base = base[:, W:].cpu().tolist()
    eos = base[0][1]
    _, out = _gen(model, g, seed=11, eos_token_id=eos, pad_token_id=0, **kw)
    new = out[:, W:].cpu().tolist()
    for b in range(len(new)):
        if eos in new[b]:
            j = new[b].index(eos)
            assert new[b][:j + 1] == base[b][:j + 1] and all(t == 0 for t in new[b][j + 1:])
        else:
            assert new[b] == base[b][:len(new[b])]
    assert new[0][:2] == base[0][:2]


def test_greedy_with_repetition_penalty(af3):
    model, g = af3
    ids, o = _gen(model, g, max_new_tokens=5, repetition_penalty=1.3, return_dict_in_generate=True, output_logits=True)
    W = ids.shape[1]
    seqs = o.sequences.cpu()
    for s, lg in enumerate(o.logits):
        for b in range(seqs.shape[0]):
            x, _ = R.process(lg[b].cpu().numpy(), penalty=1.3, ids=seqs[b, :W + s].numpy())
            assert int(seqs[b, W + s]) == R.argmax_first(x)
    # no penalty and no sampling: the greedy path, unchanged
    _, plain = _gen(model, g, max_new_tokens=g["n_steps"], do_sample=False)
    assert plain[:, W:].cpu().tolist() == np.array(g["left"]["greedy_ids"]).T.tolist()


def test_bf16_sampling_runs_and_stays_finite():
    model, g = _build(torch.bfloat16)
    ids, o = _gen(model, g, seed=1, do_sample=True, temperature=0.8, top_p=0.9, max_new_tokens=4, return_dict_in_generate=True, output_scores=True)
    assert o.sequences.shape[1] > ids.shape[1]
    for sc in o.scores:
        fin = torch.isfinite(sc)
        assert bool(fin.any(-1).all()) and not bool(torch.isnan(sc).any())


def test_unsupported_knob_raises(af3):
    model, g = af3
    for kw in (dict(min_p=0.1), dict(num_beams=2), dict(no_repeat_ngram_size=2), dict(typical_p=0.5)):
        with pytest.raises(NotImplementedError):
            _gen(model, g, do_sample=True, max_new_tokens=2, **kw)


def test_ualm_audio_topk_above_64_with_cfg():
    """audio-output decode with topk = 100 (> afhip_sample_topk's 64) and cfg = 3: every drawn code lies in the top 100 of the
    guidance-mixed, masked logits recomputed on the CPU, and a seeded run repeats."""
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    model, pre = H.build_tiny_ualm(torch.float32, DEV)
    with open(__import__("os").path.join(H.GOLD_DIR, "golden_gen.json")) as f:
        prompt = __import__("json").load(f)["cfg_sampling"]["prompt"]
    b = pre.collate_fn([(("caption_to_audio", "x", "y"), {"text": [["user", "text", prompt]]})])
    kw = {"seqs": b["seqs"].to(DEV)}
    cfg = {"audio": {"temperature": 0.8, "topk": 100, "cfg": 3.0, "max_step": 6}, "num_hypo": 1}
    rec = []
    orig = model._topk_probs

    def spy(logits, allowed, topk, temperature, cfg_logits=None, cfg=1.0, model_dtype=None, u=None):
        out = orig(logits, allowed, topk, temperature, cfg_logits=cfg_logits, cfg=cfg, model_dtype=model_dtype, u=u)
        rec.append((logits.cpu(), cfg_logits.cpu(), allowed.cpu(), out[3].cpu()))
        return out

    model._topk_probs = spy
    try:
        torch.manual_seed(0)
        hyps, _ = model.inference_segment(cfg, cache=None, enforce_modality="audio", **kw)
    finally:
        del model._topk_probs
    assert len(rec) >= 1
    for lg, cl, iv, tok in rec:
        mixed = torch.from_numpy(R.mix_f32(lg.numpy(), cl.numpy(), 3.0))
        for r in range(mixed.shape[0]):
            row = torch.full_like(mixed[r], float("-inf"))
            for lo, hi in iv[r].tolist():
                row[lo:hi] = mixed[r, lo:hi]
            _, keep = R.process(row.numpy(), temperature=0.8, top_k=100, exact_k=True)
            assert keep[int(tok[r])], (r, int(tok[r]))
    torch.manual_seed(0)
    again, _ = model.inference_segment(cfg, cache=None, enforce_modality="audio", **kw)
    assert torch.equal(hyps[0][0], again[0][0])


def test_ualm_topk_probs_above_64_draws_and_above_v_is_an_error():
    """`_topk_probs` (the decode loop's sampler call) with k = 65 (> afhip_sample_topk's 64) draws through afhip_sample_filter's exact
    top-k: the id lies in the row's top 65; k above the vocabulary is a clear ValueError."""
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    model, _ = H.build_tiny_ualm(torch.float32, DEV)
    V = len(model.vocab)
    rows = torch.randn(8, V, device=DEV)
    whole = torch.tensor([[[0, V]]], dtype=torch.int32, device=DEV).expand(8, 1, 2).contiguous()
    u = torch.rand(8, device=DEV)
    idx, val, prob, tok = model._topk_probs(rows, whole, 65, 0.8, model_dtype=torch.float32, u=u)
    assert idx is None and tok.shape == (8,)
    top = torch.topk(rows.cpu(), 65, dim=-1).indices
    for s in range(8):
        assert int(tok[s]) in top[s].tolist()
    with pytest.raises(ValueError, match="must be in"):
        model._topk_probs(rows, whole, V + 1, 0.8, model_dtype=torch.float32, u=u)
