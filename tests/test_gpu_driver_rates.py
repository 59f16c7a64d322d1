"""The inference driver (scripts/inference.py:136-153, 270-304) over samples at several sample rates: audio above 16 kHz is resampled
on the GPU by the front end and answered like the same clip resampled in float64 and fed at 16 kHz; audio below 16 kHz is still
refused per sample (the front end converts down only), and neither stops the shard."""
import numpy as np
import pytest
import torch

from oracle import fixtures_common as fc
from tests import helpers as H
from tests import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = {"text": {"temperature": 0.0, "topk": 20, "cfg": 1, "max_step": fc.MAX_STEP}, "num_hypo": 1}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")


def _sample(name, wav, fs, prompt):
    return (("audio_to_caption", "synthetic", name), {"audio": (wav[None], fs), "text": [["user", "text", prompt]]})


def test_driver_answers_44k_audio_and_refuses_8k():
    _need_gpu()
    from audio_intelligence_amd import inference as inf
    model, pre = H.build_tiny_ualm(torch.float32, DEV)
    prompt = fc.make_prompt(H.tiny_llm()[0]["text_vocab"])
    wav44 = fc.make_wav(1004, 44100 * 8 + 3)
    samples = [_sample("music", wav44, 44100, prompt),
               _sample("tel", fc.make_wav(1003, 8000 * 4), 8000, prompt),
               _sample("clip0", fc.make_wav(1000, 160000), 16000, prompt),
               _sample("music16", R.resample_f64(wav44, 44100, 16000).astype(np.float32), 16000, prompt)]
    res = inf.run_inference(model, pre, samples, CFG, device=DEV, dtype=torch.float32, enforce_modality="text")
    assert list(res.keys()) == ["music", "tel", "clip0", "music16"]
    assert "error" in res["tel"]
    role, modality, ids = res["music"][0]
    assert role == "assistant" and modality == "text" and len(ids) > 0
    assert [row[0] for row in ids] == [row[0] for row in res["music16"][0][2]]
    assert [row[0] for row in res["clip0"][0][2]] == H.golden()[0]["llm_tiny"]["greedy_tokens"][0]


def test_front_end_refuses_input_below_16k():
    _need_gpu()
    model, _ = H.build_tiny_ualm(torch.float32, DEV)
    io = model.multimodal_io_dict["continuous_audio"]
    with pytest.raises(ValueError, match="8000 < 16000"):
        io.preprocess((fc.make_wav(1, 8000), 8000))
    with pytest.raises(ValueError, match="11025 < 16000"):
        io.encode_wav_batch(torch.zeros((1, 11025), device=DEV), sample_rate=11025)
