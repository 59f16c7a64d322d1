"""afhip_sample_filter without a GPU: the test oracle (tests/sample_ref.py) against transformers' own logits processors, the ctypes
mirror of afhip_sample_filter_args against the header, argument validation (no launch), and generate()'s knob handling."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "afhip.h")


def _hf_pipeline(row, ids, pen, T, k, p):
    from transformers.generation.logits_process import (LogitsProcessorList, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    procs = LogitsProcessorList()
    if pen != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=pen))
    if T != 1.0:
        procs.append(TemperatureLogitsWarper(T))
    if k:
        procs.append(TopKLogitsWarper(top_k=k))
    if p < 1.0:
        procs.append(TopPLogitsWarper(top_p=p))
    return procs(torch.tensor(ids)[None], torch.from_numpy(row)[None].clone())[0].numpy()


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("pen,T,k,p", [(1.05, 0.7, 20, 0.8), (1.0, 1.0, 0, 0.95), (1.3, 1.0, 0, 1.0), (1.0, 0.5, 300, 1.0), (1.2, 1.3, 50, 0.5)])
def test_oracle_matches_transformers_processors(seed, pen, T, k, p):
    rng = np.random.default_rng(seed)
    V = 3000
    row = (rng.standard_normal(V) * 3).astype(np.float32)
    ids = rng.integers(0, V, 40).tolist() + [7, 7, 7]                    # repeats: the penalty applies once per distinct id
    ours, keep = R.process(row, penalty=pen, ids=ids, temperature=T, top_k=k, top_p=p)
    if p < 1.0:
        _, keep_k = R.process(row, penalty=pen, ids=ids, temperature=T, top_k=k)
        x = R.process(row, penalty=pen, ids=ids, temperature=T)[0]
        assert R.p_margin(x, keep_k, p) > 1e-6, "seeded row too close to the top-p boundary"
    hf = _hf_pipeline(row, ids, pen, T, k, p)
    assert np.array_equal(np.isfinite(hf), keep)
    np.testing.assert_array_equal(ours[keep], hf[keep])                     # element-wise steps in f32, as torch does them


def test_oracle_exact_topk_and_draw():
    x = np.array([1.0, 3.0, 3.0, 2.0, 3.0, -1.0], dtype=np.float32)
    _, keep_hf = R.process(x, top_k=2)
    _, keep_ex = R.process(x, top_k=2, exact_k=True)
    assert keep_hf.tolist() == [False, True, True, False, True, False]     # ties at the k-th value all kept
    assert keep_ex.tolist() == [False, True, True, False, False, False]    # exactly k, smaller ids first
    s, _ = R.process(x, top_k=2, exact_k=True)
    assert R.draw(s, 0.25)[0] == 1 and R.draw(s, 0.75)[0] == 2             # ascending id order, equal halves


def _header_struct_fields(cname):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\}\s*" + cname + ";", src).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            for part in decl.split(","):
                fields.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip())[0])
    return fields


def test_sample_filter_args_layout_matches_header(tmp_path):
    import shutil
    import subprocess
    from audio_intelligence_amd import _lib as L
    assert _header_struct_fields("afhip_sample_filter_args") == [f[0] for f in L.SampleFilterArgs._fields_]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler on this host")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(afhip_sample_filter_args));']
    for fname, _ in L.SampleFilterArgs._fields_:
        lines.append(f'  printf("{fname} %zu %zu\\n", offsetof(afhip_sample_filter_args, {fname}), sizeof(((afhip_sample_filter_args*)0)->{fname}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run([cc, "-std=c11", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict((ln.split()[0], tuple(int(v) for v in ln.split()[1:])) for ln in
               subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert got["size"] == (C.sizeof(L.SampleFilterArgs),)
    for fname, _ in L.SampleFilterArgs._fields_:
        fd = getattr(L.SampleFilterArgs, fname)
        assert got[fname] == (fd.offset, fd.size), fname


def _valid_args(L, ws_ok=True):
    a = L.SampleFilterArgs()
    a.logits, a.rows, a.V, a.ld = 0x1000, 4, 3000, 3000
    a.model_dtype, a.penalty, a.temperature, a.top_k, a.top_p = L.F32, 1.0, 1.0, 0, 1.0
    a.u, a.token = 0x2000, 0x3000
    return a


@pytest.mark.parametrize("field,value,msg", [
    ("logits", None, "null logits"), ("rows", 0, "bad shape"), ("ld", 10, "bad shape"), ("V", 1 << 23, "bad shape"),
    ("top_k", 3001, "top_k"), ("top_k", -1, "top_k"), ("temperature", 0.0, "temperature"), ("temperature", -1.0, "temperature"),
    ("top_p", 0.0, "top_p"), ("top_p", 1.5, "top_p"), ("penalty", 0.0, "penalty"), ("model_dtype", 7, "model_dtype"),
    ("n_iv", 0, "n_iv")])
def test_sample_filter_rejects_bad_arguments_without_launching(field, value, msg):
    from audio_intelligence_amd import _lib as L
    lib = L.load_library()
    a = _valid_args(L)
    if field == "n_iv":
        a.allowed = 0x4000
    setattr(a, field, value)
    need = lib.afhip_sample_filter_workspace_bytes(4, 3000)
    assert need > 0
    rc = lib.afhip_sample_filter(C.byref(a), C.c_void_p(1 << 20), need, None)
    assert rc != 0 and msg in lib.afhip_last_error().decode()


def test_sample_filter_rejects_small_workspace_and_penalty_without_counts():
    from audio_intelligence_amd import _lib as L
    lib = L.load_library()
    a = _valid_args(L)
    need = lib.afhip_sample_filter_workspace_bytes(4, 3000)
    assert lib.afhip_sample_filter(C.byref(a), C.c_void_p(1 << 20), need - 1, None) != 0
    assert "workspace" in lib.afhip_last_error().decode()
    assert lib.afhip_sample_filter(C.byref(a), None, need, None) != 0
    a.penalty, a.penalty_ids = 1.1, 0x5000
    assert lib.afhip_sample_filter(C.byref(a), C.c_void_p(1 << 20), need, None) != 0
    assert "n_ids" in lib.afhip_last_error().decode()
    assert lib.afhip_sample_filter(None, C.c_void_p(1 << 20), need, None) != 0
    assert lib.afhip_sample_filter_workspace_bytes(0, 3000) == 0
    assert lib.afhip_sample_filter_workspace_bytes(16, 152064) >= 16 * 152064 * 4


def test_generate_knobs_merge_and_reject():
    from transformers import GenerationConfig
    from audio_intelligence_amd.multimodal_io.qwen2_audio_generation import _generation_knobs
    k = _generation_knobs(GenerationConfig(do_sample=True, top_k=5, top_p=0.5), {}, top_p=0.9)
    assert k["do_sample"] is True and k["top_k"] == 5 and k["top_p"] == 0.9              # explicit kwargs win
    assert _generation_knobs({"temperature": 0.7}, {})["temperature"] == 0.7
    assert _generation_knobs(None, {"num_beams": 1, "typical_p": 1.0})["top_k"] is None   # neutral values are accepted
    for knob, v in (("min_p", 0.1), ("typical_p", 0.9), ("num_beams", 4), ("no_repeat_ngram_size", 3)):
        with pytest.raises(NotImplementedError, match=knob):
            _generation_knobs(None, {knob: v})
    with pytest.raises(NotImplementedError, match="min_p"):
        _generation_knobs(GenerationConfig(min_p=0.2), {})
    with pytest.raises(TypeError):
        _generation_knobs(None, {"not_a_knob": 1})
