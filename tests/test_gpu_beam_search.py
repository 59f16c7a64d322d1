"""Beam search on the GPU: afhip_beam_select against a float64 oracle and its own log-prob output, afhip_kv_gather bit-exact against
index_select, and generate(num_beams=...) on the tiny AF3 model of test_gpu_af3.py replayed through tests/beam_ref.py and rescored by
teacher-forced forward() passes."""
import numpy as np
import pytest
import torch

from tests import beam_ref as BR
from tests.test_gpu_af3 import _build, _inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from audio_intelligence_amd import ops
    return ops


# ---------------------------------------------------------------- afhip_beam_select

def _select_inputs(B, nb, V, seed, hf_init):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B * nb, V), generator=g) * 3
    x[:, torch.randint(0, V, (V // 50,), generator=g)] = -float("inf")            # -inf logits
    x[0, 1:40:3] = x[0, 0]                                                      # exact ties inside a row
    if hf_init:                                                                 # HF's first step: beam 0 live, the rest at -1e9
        run = torch.full((B, nb), -1e9)
        run[:, 0] = 0
    else:
        run = -torch.rand((B, nb), generator=g) * 6
    return x, run


def _own_topk(own, K):
    """top K of a [B, N] f32 array under (value descending, index ascending)"""
    out = []
    for row in own:
        order = np.lexsort((np.arange(row.size), -row.astype(np.float64)))
        out.append(order[:K])
    return np.stack(out)


SHAPES = [(2, 1, 3000, 2, False, True), (2, 2, 3000, 4, True, True), (3, 4, 152064, 8, False, True), (2, 4, 152064, 12, True, False),
          (1, 8, 8192 * 3 + 17, 16, False, False), (2, 16, 8192 * 3 + 17, 128, True, True), (1, 32, 152064, 64, False, False),
          (2, 32, 3000, 128, False, True), (4, 2, 152064, 4, True, False), (1, 1, 152064, 128, True, False)]


@pytest.mark.parametrize("B,nb,V,K,bf16,hf_init", SHAPES)
def test_beam_select_against_float64_and_itself(B, nb, V, K, bf16, hf_init):
    ops = _ops()
    x, run = _select_inputs(B, nb, V, seed=B * 1000 + nb * 10 + K, hf_init=hf_init)
    xd, rd = x.to(DEV), run.to(DEV)
    md = torch.bfloat16 if bf16 else torch.float32
    sc = torch.empty((B * nb, V), dtype=torch.float32, device=DEV)
    vals, idx = ops.beam_select(xd, rd, K, model_dtype=md, scores=sc)
    vals2, idx2 = ops.beam_select(xd, rd, K, model_dtype=md, scores=sc.clone())
    vals3, idx3 = ops.beam_select(xd, rd, K, model_dtype=md)
    torch.cuda.synchronize()
    # bit-identical across launches and with / without the log-prob rows
    assert torch.equal(idx, idx2) and torch.equal(idx, idx3)
    assert torch.equal(vals.view(torch.int32), vals2.view(torch.int32)) and torch.equal(vals.view(torch.int32), vals3.view(torch.int32))
    vals, idx, sc = vals.cpu(), idx.cpu(), sc.cpu()
    # exact self-consistency: top K of the kernel's own log-probs + running, in the stated order, with the same values
    own = (sc.view(B, nb, V) + run[:, :, None]).reshape(B, nb * V)
    want = _own_topk(own.numpy(), K)
    assert np.array_equal(idx.numpy(), want)
    assert torch.equal(vals.view(torch.int32), torch.gather(own, 1, idx).view(torch.int32))
    # float64 oracle: values to 1e-6 relative, index sets wherever the gap at the K-th candidate is wider than that
    xr = x.bfloat16().double() if bf16 else x.double()
    lp64 = torch.log_softmax(xr, -1)
    fin = torch.isfinite(lp64)
    assert torch.equal(fin, torch.isfinite(sc))
    assert float(((sc.double() - lp64)[fin]).abs().max()) <= 1e-6 * max(1.0, float(lp64[fin].abs().max()))
    c64 = (lp64.view(B, nb, V) + run.double()[:, :, None]).reshape(B, nb * V)
    got64 = torch.gather(c64, 1, idx)
    ok = torch.isfinite(got64)
    assert torch.equal(ok, torch.isfinite(vals))
    tol = 1e-6 * got64[ok].abs().clamp(min=1.0)
    assert bool(((vals.double()[ok] - got64[ok]).abs() <= tol).all())
    s64 = torch.sort(c64, -1, descending=True)[0]
    for b in range(B):
        gap = float(s64[b, K - 1] - s64[b, K]) if K < nb * V else float("inf")
        if gap > 1e-6 * max(1.0, abs(float(s64[b, K - 1]))):
            assert set(idx[b].tolist()) == set(torch.topk(c64[b], K)[1].tolist()), b


def test_beam_select_ties_from_rounding_go_to_the_smaller_flat_index():
    """running = -1e9 swallows every log-prob difference below 32: the candidates tie and the smaller flat index wins"""
    ops = _ops()
    B, nb, V, K = 1, 4, 20000, 8
    x = torch.randn((B * nb, V)) * 0.5
    run = torch.full((B, nb), -1e9)
    vals, idx = ops.beam_select(x.to(DEV), run.to(DEV), K)
    vals, idx = vals.cpu(), idx.cpu()
    assert bool((vals == -1e9).all())
    assert idx[0].tolist() == list(range(K))


# ---------------------------------------------------------------- afhip_kv_gather

def _kv(n_l, B, nkv, cap, hd, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((n_l, B, nkv, cap, hd), generator=g) * 4).to(dtype).to(DEV) for _ in range(2)]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


MAPS = {"identity": [0, 1, 2, 3, 4, 5], "swaps": [1, 0, 3, 2, 5, 4], "3-cycles": [1, 2, 0, 4, 5, 3], "all-from-one": [2] * 6,
        "mixed": [3, 3, 0, 1, 4, 0]}


@pytest.mark.parametrize("dims", [(2, 2, 64, 64), (28, 4, 320, 128)], ids=["tiny", "7B"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("name", list(MAPS))
def test_kv_gather_bit_exact(dims, dtype, in_place, name):
    ops = _ops()
    n_l, nkv, cap, hd = dims
    B = 6
    parent = torch.tensor(MAPS[name], dtype=torch.int32)
    g = torch.Generator().manual_seed(len(name))
    row0 = torch.randint(0, cap // 4, (B,), generator=g, dtype=torch.int32)
    row1 = (row0 + torch.randint(0, cap // 2, (B,), generator=g, dtype=torch.int32)).clamp(max=cap)
    row1[4] = row0[4]                                                            # an empty range
    max_rows = int((row1 - row0).max())
    sk, sv = _kv(n_l, B, nkv, cap, hd, dtype, 1)
    if in_place:
        dk, dv = sk, sv
    else:
        dk, dv = _kv(n_l, B, nkv, cap, hd, dtype, 2)                            # sentinels: every untouched row keeps its bits
    want_k, want_v = dk.clone(), dv.clone()
    src_k, src_v = sk.clone(), sv.clone()
    for r in range(B):
        a, b = int(row0[r]), int(row1[r])
        want_k[:, r, :, a:b] = torch.index_select(src_k, 1, parent[r:r + 1].long().to(DEV))[:, 0, :, a:b]
        want_v[:, r, :, a:b] = torch.index_select(src_v, 1, parent[r:r + 1].long().to(DEV))[:, 0, :, a:b]
    ops.kv_gather(sk, sv, dk, dv, parent.to(DEV), row0.to(DEV), row1.to(DEV), max_rows)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dk), _bits(want_k)) and torch.equal(_bits(dv), _bits(want_v))
    if not in_place:
        assert torch.equal(_bits(sk), _bits(src_k)) and torch.equal(_bits(sv), _bits(src_v))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_kv_gather_expands_b_prompts_to_b_times_nb_slots(dtype):
    ops = _ops()
    n_l, nkv, cap, hd, B, nb = 28, 4, 256, 128, 2, 4
    sk, sv = _kv(n_l, B, nkv, cap, hd, dtype, 3)
    dk, dv = _kv(n_l, B * nb, nkv, cap, hd, dtype, 4)
    lens = torch.tensor([200, 137], dtype=torch.int32)
    parent = torch.arange(B * nb, dtype=torch.int32) // nb
    row1 = lens.repeat_interleave(nb)
    want_k, want_v = dk.clone(), dv.clone()
    ik = torch.index_select(sk, 1, parent.long().to(DEV))
    iv = torch.index_select(sv, 1, parent.long().to(DEV))
    for r in range(B * nb):
        want_k[:, r, :, :int(row1[r])] = ik[:, r, :, :int(row1[r])]
        want_v[:, r, :, :int(row1[r])] = iv[:, r, :, :int(row1[r])]
    ops.kv_gather(sk, sv, dk, dv, parent.to(DEV), torch.zeros(B * nb, dtype=torch.int32, device=DEV), row1.to(DEV), 200)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dk), _bits(want_k)) and torch.equal(_bits(dv), _bits(want_v))


# ---------------------------------------------------------------- generate(num_beams=...)

@pytest.fixture(scope="module")
def af3():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return _build()


def _run(model, g, side, **kw):
    ids, mask, feats, fmask = _inputs(g, side)
    model.padding_side = side
    try:
        o = model.generate(ids, input_features=feats, attention_mask=mask, feature_attention_mask=fmask, **kw)
    finally:
        model.padding_side = "left"
    return (ids, mask, feats, fmask), o


def _rescore(model, inputs, o, nrs, lp):
    """each hypothesis through a fresh teacher-forced forward(): summed log-probs of its generated tokens / len ** length_penalty"""
    ids, mask, feats, fmask = inputs
    W = ids.shape[1]
    out = []
    for i in range(o.sequences.shape[0]):
        b = i // nrs
        n = int((o.beam_indices[i] != -1).sum())
        toks = o.sequences[i, W:W + n].cpu()
        seq = torch.cat([ids[b][mask[b].bool()], toks])[None]
        f = model.forward(input_ids=seq, input_features=feats[b:b + 1], attention_mask=torch.ones_like(seq),
                          feature_attention_mask=fmask[b:b + 1], use_cache=False)
        rows = f.logits[0][f.attention_mask[0].to(DEV).bool()][-(n + 1):-1].float()
        lps = torch.log_softmax(rows, -1).gather(1, toks.to(DEV)[:, None])[:, 0]
        out.append(float(lps.double().sum()) / (n ** lp))
    return torch.tensor(out, dtype=torch.float64)


def _replay(o, inputs, V, nb, n_new, nrs, eos, pad, lp, es):
    ids = inputs[0]
    logits = [t.cpu() for t in o.logits]

    def fn(step, seqs):
        return logits[step] if step < len(logits) else torch.zeros((seqs.shape[0], V))
    return BR.beam_search(fn, ids, V, nb, n_new, eos=eos, pad=pad, length_penalty=lp, early_stopping=es, num_return_sequences=nrs)


def _check(model, g, side, nb=4, nrs=2, n_new=6, eos=(), lp=1.0, es=False, score_tol=2e-3):
    kw = dict(num_beams=nb, num_return_sequences=nrs, max_new_tokens=n_new, length_penalty=lp, early_stopping=es,
              return_dict_in_generate=True, output_scores=True, output_logits=True)
    if eos:
        kw["eos_token_id"] = list(eos)
    inputs, o = _run(model, g, side, **kw)
    B, W = inputs[0].shape
    V = g["text_cfg"]["vocab_size"]
    assert o.sequences.shape[0] == B * nrs and o.beam_indices.shape[0] == B * nrs
    assert o.sequences.shape[1] == W + o.beam_indices.shape[1] <= W + n_new
    assert torch.equal(o.sequences[:, :W].cpu(), inputs[0].repeat_interleave(nrs, 0))
    assert len(o.scores) == len(o.logits) >= 1 and o.scores[0].shape == (B * nb, V)
    for sc, lg in zip(o.scores, o.logits):                                       # every step's log-prob rows
        torch.testing.assert_close(sc.cpu(), torch.log_softmax(lg.cpu().float(), -1), rtol=0, atol=1e-5)
    # replay through the host restatement, driven by the GPU's own per-step logits
    ref = _replay(o, inputs, V, nb, n_new, nrs, list(eos), model.pad_token_id, lp, es)
    if ref.margin > 1.5e-5:                                     # a few f32 ulps of the summed scores: no choice can flip
        assert len(ref.scores) == len(o.scores)
        assert torch.equal(o.sequences.cpu(), ref.sequences)
        assert torch.equal(o.beam_indices.cpu(), ref.beam_indices)
        torch.testing.assert_close(o.sequences_scores.cpu(), ref.sequences_scores, rtol=1e-6, atol=1e-5)
    # rescoring: what catches a wrong cache reorder
    rs = _rescore(model, inputs, o, nrs, lp)
    assert float((rs - o.sequences_scores.cpu().double()).abs().max()) <= score_tol, (rs, o.sequences_scores)
    return inputs, o, ref


@pytest.mark.parametrize("side", ["left", "right"])
def test_generate_beam_replay_and_rescore(af3, side):
    model, g = af3
    _, o, ref = _check(model, g, side)
    assert ref.margin > 1.5e-5, "seeded run too close to a tie for the replay"
    assert bool((o.beam_indices[:, 1:] != -1).any())            # beams moved between slots: the reorder was exercised
    hops = set()
    for row in o.beam_indices.cpu().tolist():
        hops.update(b % 4 for b in row if b >= 0)
    assert len(hops) > 1


@pytest.mark.parametrize("lp,es", [(1.0, True), (0.0, "never"), (2.0, "never"), (-1.0, False)])
def test_generate_beam_early_stopping_variants(af3, lp, es):
    model, g = af3
    _check(model, g, "left", nb=3, nrs=3, lp=lp, es=es)


def test_generate_beam_eos_forces_early_finishes(af3):
    model, g = af3
    inputs, o = _run(model, g, "left", num_beams=4, max_new_tokens=6)
    W = inputs[0].shape[1]
    eos = [int(o[0, W + 1]), int(o[1, W])]
    _, o2, _ = _check(model, g, "left", nb=4, nrs=4, eos=eos)
    n = (o2.beam_indices != -1).sum(1)
    assert int(n.min()) < 6                                      # some hypothesis ended on an eos before max_length
    fill = eos[0]                                                # pad id 0 falls through to eos[0]
    for i in range(o2.sequences.shape[0]):
        assert bool((o2.sequences[i, W + int(n[i]):] == fill).all())


def test_generate_beam_plain_call_and_single_beam_unchanged(af3):
    model, g = af3
    inputs, plain = _run(model, g, "left", num_beams=4, num_return_sequences=2, max_new_tokens=6)
    _, full = _run(model, g, "left", num_beams=4, num_return_sequences=2, max_new_tokens=6, return_dict_in_generate=True)
    assert torch.equal(plain, full.sequences) and full.sequences_scores is None and full.scores is None
    _, one = _run(model, g, "left", num_beams=1, max_new_tokens=g["n_steps"])
    assert one[:, inputs[0].shape[1]:].cpu().tolist() == np.array(g["left"]["greedy_ids"]).T.tolist()


def test_generate_beam_bf16():
    model, g = _build(torch.bfloat16)
    _check(model, g, "left", score_tol=0.15)


def test_generate_beam_rejects_what_it_does_not_serve(af3):
    model, g = af3
    with pytest.raises(NotImplementedError):
        _run(model, g, "left", do_sample=True, num_beams=2, max_new_tokens=2)
    with pytest.raises(NotImplementedError):
        _run(model, g, "left", num_beams=2, repetition_penalty=1.2, max_new_tokens=2)
    with pytest.raises(ValueError):
        _run(model, g, "left", num_beams=2, num_return_sequences=3, max_new_tokens=2)
