"""Beam search without a GPU: tests/beam_ref.py pinned to transformers' own generate(num_beams=...) on a small float64 Qwen2, the ctypes
mirror of afhip_beam_select_args against the C compiler, argument validation of both beam entry points (no launch), and generate()'s
beam-knob handling."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import beam_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "afhip.h")
V = 300


@pytest.fixture(scope="module")
def qwen2():
    from transformers import Qwen2Config, Qwen2ForCausalLM
    cfg = Qwen2Config(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      max_position_embeddings=64, rope_theta=10000.0, rms_norm_eps=1e-6, tie_word_embeddings=False, attn_implementation="sdpa",
                      pad_token_id=None, bos_token_id=None, eos_token_id=None)
    g = torch.Generator().manual_seed(5)
    m = Qwen2ForCausalLM(cfg).double().eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_((1 + 0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64)) if n.endswith("norm.weight")
                    else 0.35 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    return m


def _logits_fn(m, mask0):
    """the model over the full running sequences (no cache), as HF feeds them: mask extended with ones, positions cumsum(mask) - 1"""
    def fn(step, seqs):
        nb = seqs.shape[0] // mask0.shape[0]
        mask = torch.cat([mask0.repeat_interleave(nb, 0), torch.ones((seqs.shape[0], step), dtype=mask0.dtype)], 1)
        pos = (mask.cumsum(-1) - 1).masked_fill(mask == 0, 1)
        with torch.no_grad():
            return m(input_ids=seqs, attention_mask=mask, position_ids=pos).logits[:, -1]
    return fn


def _prompts(batch):
    g = torch.Generator().manual_seed(17)
    if batch == 1:
        return torch.randint(0, V, (1, 5), generator=g), torch.ones((1, 5), dtype=torch.long)
    ids = torch.randint(0, V, (2, 6), generator=g)
    mask = torch.ones((2, 6), dtype=torch.long)
    ids[1, :2], mask[1, :2] = 0, 0                               # left-padded second prompt
    return ids, mask


CASES = [dict(nb=2, eos=(), es=False, lp=1.0, nrs=1, batch=1), dict(nb=4, eos=(), es=False, lp=1.0, nrs=4, batch=1),
         dict(nb=4, eos="one", es=True, lp=1.0, nrs=1, batch=1), dict(nb=2, eos="two", es=False, lp=0.0, nrs=2, batch=1),
         dict(nb=4, eos="one", es="never", lp=2.0, nrs=4, batch=1), dict(nb=4, eos="two", es="never", lp=-1.0, nrs=1, batch=1),
         dict(nb=2, eos="one", es=True, lp=0.0, nrs=2, batch=1), dict(nb=4, eos="one", es=False, lp=1.0, nrs=2, batch=2),
         dict(nb=2, eos="two", es="never", lp=1.0, nrs=1, batch=2), dict(nb=4, eos=(), es=True, lp=2.0, nrs=4, batch=2)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "nb{nb}-eos{eos}-es{es}-lp{lp}-nrs{nrs}-b{batch}".format(**c))
def test_beam_ref_matches_transformers_generate(qwen2, case):
    ids, mask = _prompts(case["batch"])
    nb, n_new = case["nb"], 8
    # eos ids that the search actually meets: the greedy continuation's own tokens
    with torch.no_grad():
        greedy = qwen2.generate(ids, attention_mask=mask, max_new_tokens=4, do_sample=False, pad_token_id=0)[0, ids.shape[1]:].tolist()
    eos = {(): [], "one": [greedy[1]], "two": [greedy[2], greedy[0]]}[case["eos"]]
    kw = dict(num_beams=nb, num_return_sequences=case["nrs"], length_penalty=case["lp"], early_stopping=case["es"], max_new_tokens=n_new,
              do_sample=False, pad_token_id=7, eos_token_id=eos or None, return_dict_in_generate=True, output_scores=True)
    with torch.no_grad():
        hf = qwen2.generate(ids, attention_mask=mask, **kw)
    ref = BR.beam_search(_logits_fn(qwen2, mask), ids, V, nb, n_new, eos=eos, pad=7, length_penalty=case["lp"],
                         early_stopping=case["es"], num_return_sequences=case["nrs"])
    assert ref.margin > 1e-6
    assert torch.equal(ref.sequences, hf.sequences)
    assert torch.equal(ref.beam_indices, hf.beam_indices.to(ref.beam_indices.dtype))
    torch.testing.assert_close(ref.sequences_scores, hf.sequences_scores, rtol=1e-6, atol=1e-6)


def test_beam_ref_fill_value_follows_pad_or_eos():
    """a finished hypothesis shorter than the longest is filled with `pad or eos[0]` (a pad id of 0 falls through), -1 without eos"""
    ids = torch.tensor([[3, 4]])
    V_ = 6

    def fn(step, seqs):                                           # beam 0 ends at once on id 5; the other runs to max_length
        x = torch.full((seqs.shape[0], V_), -5.0)
        x[:, 5] = 2.0 if step == 0 else -9.0
        x[:, 1] = 1.5
        return x
    for pad, want in ((0, 5), (2, 2)):
        r = BR.beam_search(fn, ids, V_, 2, 3, eos=[5], pad=pad, num_return_sequences=2)
        short = [s for s, bi in zip(r.sequences.tolist(), r.beam_indices.tolist()) if bi.count(-1) > 0]
        assert short and all(t == want for t in short[0][3:])
    r = BR.beam_search(fn, ids, V_, 2, 3, pad=0)
    assert r.sequences.shape == (1, 5)


def _header_struct_fields(cname):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\}\s*" + cname + ";", src).group(1)
    return [re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip())[0] for decl in body.split(";") if decl.strip()
            for part in decl.strip().split(",")]


def test_beam_select_args_layout_matches_the_c_compiler(tmp_path):
    import shutil
    import subprocess
    from audio_intelligence_amd import _lib as L
    assert _header_struct_fields("afhip_beam_select_args") == [f[0] for f in L.BeamSelectArgs._fields_]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler on this host")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(afhip_beam_select_args));']
    for fname, _ in L.BeamSelectArgs._fields_:
        lines.append(f'  printf("{fname} %zu %zu\\n", offsetof(afhip_beam_select_args, {fname}), sizeof(((afhip_beam_select_args*)0)->{fname}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run([cc, "-std=c11", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict((ln.split()[0], tuple(int(v) for v in ln.split()[1:])) for ln in
               subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert got["size"] == (C.sizeof(L.BeamSelectArgs),)
    for fname, _ in L.BeamSelectArgs._fields_:
        fd = getattr(L.BeamSelectArgs, fname)
        assert got[fname] == (fd.offset, fd.size), fname


def _valid_select(L):
    a = L.BeamSelectArgs()
    a.logits, a.model_dtype, a.B, a.nb, a.V, a.ld = 0x1000, L.F32, 2, 4, 3000, 3000
    a.running, a.K, a.values, a.indices = 0x2000, 8, 0x3000, 0x4000
    return a


@pytest.mark.parametrize("field,value,msg", [
    ("logits", None, "null logits"), ("values", None, "null values"), ("nb", 0, "nb="), ("nb", 33, "nb="), ("B", 0, "bad shape"),
    ("V", 1 << 23, "bad shape"), ("ld", 10, "bad shape"), ("K", 0, "K="), ("K", 129, "K="), ("model_dtype", 7, "model_dtype")])
def test_beam_select_rejects_bad_arguments_without_launching(field, value, msg):
    from audio_intelligence_amd import _lib as L
    lib = L.load_library()
    a = _valid_select(L)
    setattr(a, field, value)
    need = lib.afhip_beam_select_workspace_bytes(2, 4, 3000, 8)
    assert need > 0
    rc = lib.afhip_beam_select(C.byref(a), C.c_void_p(1 << 20), need, None)
    assert rc != 0 and msg in lib.afhip_last_error().decode()


def test_beam_select_rejects_small_workspace_and_k_above_the_candidates():
    from audio_intelligence_amd import _lib as L
    lib = L.load_library()
    a = _valid_select(L)
    need = lib.afhip_beam_select_workspace_bytes(2, 4, 3000, 8)
    assert lib.afhip_beam_select(C.byref(a), C.c_void_p(1 << 20), need - 1, None) != 0
    assert "workspace" in lib.afhip_last_error().decode()
    a.V, a.ld, a.nb, a.K = 10, 10, 2, 21
    assert lib.afhip_beam_select(C.byref(a), C.c_void_p(1 << 20), 1 << 20, None) != 0 and "nb * V" in lib.afhip_last_error().decode()
    assert lib.afhip_beam_select_workspace_bytes(1, 33, 3000, 8) == 0 and lib.afhip_beam_select_workspace_bytes(1, 4, 3000, 129) == 0


def test_kv_gather_rejects_bad_arguments_without_launching():
    from audio_intelligence_amd import _lib as L
    lib = L.load_library()
    s, d = L.KvCache(), L.KvCache()
    s.k, s.v, s.cap, s.B = 0x1000, 0x2000, 64, 2
    d.k, d.v, d.cap, d.B = 0x1000, 0x2000, 64, 2
    P = C.c_void_p(0x3000)
    need = lib.afhip_kv_gather_workspace_bytes(2, 2, 2, 64, 16, L.BF16)
    assert need == 2 * 2 * 2 * 2 * 16 * 64 * 2
    assert lib.afhip_kv_gather(C.byref(s), C.byref(d), 2, 2, 64, L.BF16, P, P, P, 16, C.c_void_p(1 << 20), need - 1, None) != 0
    assert "workspace" in lib.afhip_last_error().decode()
    assert lib.afhip_kv_gather(C.byref(s), C.byref(d), 2, 2, 4, L.BF16, P, P, P, 16, C.c_void_p(1 << 20), 1 << 20, None) != 0
    assert "16 bytes" in lib.afhip_last_error().decode()
    d.v = 0x5000
    assert lib.afhip_kv_gather(C.byref(s), C.byref(d), 2, 2, 64, L.BF16, P, P, P, 16, C.c_void_p(1 << 20), 1 << 20, None) != 0
    assert "both" in lib.afhip_last_error().decode()
    d.k, d.cap = 0x4000, 128
    assert lib.afhip_kv_gather(C.byref(s), C.byref(d), 2, 2, 64, L.BF16, P, P, P, 16, None, 0, None) != 0
    assert "cap" in lib.afhip_last_error().decode()
    d.cap = 64
    assert lib.afhip_kv_gather(C.byref(s), C.byref(d), 2, 2, 64, L.BF16, None, P, P, 16, None, 0, None) != 0
    # out of place needs no workspace; max_rows 0 launches nothing
    assert lib.afhip_kv_gather(C.byref(s), C.byref(d), 2, 2, 64, L.BF16, P, P, P, 0, None, 0, None) == 0


def test_beam_knobs_peel_and_leave_the_rest_alone():
    from transformers import GenerationConfig
    from audio_intelligence_amd.multimodal_io.qwen2_audio_generation import _beam_knobs, _generation_knobs
    beam, gc, kw = _beam_knobs(GenerationConfig(num_beams=4, length_penalty=0.5), {"num_return_sequences": 2, "early_stopping": "never"})
    assert beam == dict(num_beams=4, num_return_sequences=2, length_penalty=0.5, early_stopping="never")
    assert kw == {} and gc["num_beams"] == 1
    assert isinstance(_generation_knobs(gc, kw), dict)                       # the neutralised knobs pass the unchanged gate
    beam, _, _ = _beam_knobs({"num_beams": 2}, {"num_beams": 3})
    assert beam["num_beams"] == 3 and beam["early_stopping"] is False        # explicit kwargs win
    for args in (({}, {"num_beams": 1}), (None, {}), ({"num_beams": 4, "do_sample": True}, {})):
        beam, gc, kw = _beam_knobs(*args)
        assert beam is None and gc is args[0] and kw is args[1]             # untouched: single-hypothesis decoding as before
    b, _, _ = _beam_knobs(None, {"num_beams": 4}, do_sample=True)
    assert b is None
    with pytest.raises(ValueError):
        _beam_knobs(None, {"num_beams": 2, "num_return_sequences": 3})
    with pytest.raises(NotImplementedError, match="num_beams"):
        _generation_knobs(None, {"num_beams": 4})
