"""Shared test helpers: golden fixtures, seeded inputs/weights (test infrastructure)."""
import json
import os

import numpy as np
import torch

import oracle
from oracle import fixtures_common as fc
from audio_intelligence_amd.utils import synthetic as syn

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cpu_threads():
    """CPU threads this process may really use: the scheduler affinity capped by the cgroup CPU quota (a GPU box shows every core
    of the host in the affinity mask but grants a 16-CPU share; oversubscribing it makes the oracle crawl)."""
    n = len(os.sched_getaffinity(0))
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        n = min(n, 16)
    return max(1, min(n, 64))
_cache = {}


def golden():
    if "g" not in _cache:
        with open(os.path.join(GOLD_DIR, "golden.json")) as f:
            _cache["g"] = json.load(f)
        _cache["a"] = dict(np.load(os.path.join(GOLD_DIR, "golden_arrays.npz")))
    return _cache["g"], _cache["a"]


def tiny_enc():
    if "tiny_enc" not in _cache:
        cfg = oracle.afwhisper.tiny_config()
        _cache["tiny_enc"] = (cfg, syn.synth_state_dict(syn.encoder_param_shapes(cfg), fc.SEED_ENC_TINY))
    return _cache["tiny_enc"]


def tiny_llm():
    if "tiny_llm" not in _cache:
        cfg = oracle.qwen2.config_tiny()
        vocab, iv = oracle.ualm.build_vocabulary(cfg["text_vocab"])
        sd = syn.synth_state_dict(syn.llm_param_shapes(cfg, len(vocab), 8, 384), fc.SEED_LLM_TINY)
        _cache["tiny_llm"] = (cfg, sd, vocab, iv)
    return _cache["tiny_llm"]


def mel_of(seed, n):
    key = ("mel", seed, n)
    if key not in _cache:
        _cache[key] = oracle.logmel.log_mel(fc.make_wav(seed, n))
    return _cache[key]


def caption_batch(seed, n=160000, prompt=None):
    cfg, sd, vocab, iv = tiny_llm()
    if prompt is None:
        prompt = fc.make_prompt(cfg["text_vocab"])
    s = oracle.ualm.preprocessing("audio_to_caption", {"text1": np.array(prompt)}, fc.make_wav(seed, n), iv)
    return oracle.ualm.collate([s])


# ---------------------------------------------------------------------------------------------------------
# stub discrete IOs (no tokenizer / codec offline): the vocabulary contract only
def stub_ios(text_vocab):
    from audio_intelligence_amd.multimodal_io.abs_io import AbsIO

    class StubText(AbsIO):
        def __init__(self):
            super().__init__(modality="text", is_discrete=True)
            self.vocab_size = text_vocab

        def preprocess(self, data):
            t = np.array(data, dtype=np.int32).reshape(-1, 1)
            return t, None, (t * 0 + 1).astype(np.float32)

        def find_length(self, data):
            return len(data)

        def copy_for_worker(self):
            return self

        def num_stream(self):
            return 1

        def get_vocabulary(self):
            return [f"<text_{i}>" for i in range(text_vocab)]

        def get_stream_interval(self):
            return [(0, text_vocab)]

        def decode_batch(self, tokens, lengths):
            return [t[:l, 0].tolist() for t, l in zip(tokens.cpu(), lengths.cpu())]

    class StubAudio(AbsIO):
        def __init__(self):
            super().__init__(modality="audio", is_discrete=True)

        def copy_for_worker(self):
            return self

        def num_stream(self):
            return 8

        def get_vocabulary(self):
            return [f"<audio_{i}>" for i in range(8 * 1025)]

        def get_stream_interval(self):
            return [(s * 1025, (s + 1) * 1025) for s in range(8)]

    return StubText(), StubAudio()


def build_tiny_ualm(dtype=torch.float32, device="cuda:0"):
    """The drop-in stack on the GPU with the seeded synthetic weights the golden vectors were captured with."""
    import json
    import tempfile
    from audio_intelligence_amd.multimodal_io.audio import ContinuousAudioIO
    from audio_intelligence_amd.multimodal_io.modeling_whisper import AFWhisperEncoder, AFWhisperEncoderConfig
    from audio_intelligence_amd.lm.parallel import ParallelHFModel
    from audio_intelligence_amd import ualm_job
    ecfg, esd = tiny_enc()
    lcfg, lsd, vocab, iv = tiny_llm()
    enc = AFWhisperEncoder(AFWhisperEncoderConfig.from_dict(ecfg))
    enc.load_state_dict(esd, strict=True)
    text_io, audio_io = stub_ios(lcfg["text_vocab"])
    cont = ContinuousAudioIO(encoder_choice="AFWhisper", dtype=str(dtype).replace("torch.", ""), device=device, encoder=enc)
    ios = {"text": text_io, "discrete_audio": audio_io, "continuous_audio": cont}
    v2, iv2 = ualm_job.build_vocabulary(ios)
    assert v2 == vocab and iv2 == iv
    with tempfile.TemporaryDirectory() as d:
        hf = {"architectures": ["Qwen2ForCausalLM"], "hidden_size": lcfg["hidden_size"], "num_hidden_layers": lcfg["num_hidden_layers"],
              "num_attention_heads": lcfg["num_attention_heads"], "num_key_value_heads": lcfg["num_key_value_heads"],
              "intermediate_size": lcfg["intermediate_size"], "rope_theta": lcfg["rope_theta"], "rms_norm_eps": lcfg["rms_norm_eps"],
              "vocab_size": lcfg["text_vocab"]}
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump(hf, f)
        model = ParallelHFModel(d, multimodal_io=ios, vocab=vocab, vocab_intervals=iv, dtype=dtype)
    full = dict(lsd)
    for k, v in esd.items():
        full["multimodal_io_dict.continuous_audio.model." + k] = v
    res = model.load_state_dict(full, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model = model.to(device, dtype)
    model.prepare_inference()
    model.eval()
    pre = ualm_job.UALMPreprocessor(False, {k: v.copy_for_worker() for k, v in ios.items()}, vocab, iv)
    return model, pre


# ---------------------------------------------------------------------------------------------------------
# AF3-7B WIDTHS with few layers (BASELINE config 3 shape): H 3584, 28 q / 4 kv heads x 128, FFN 18944, V 160520
def stub_continuous(d_model):
    from audio_intelligence_amd.multimodal_io.abs_io import AbsIO

    class _Cont(AbsIO):
        """continuous IO whose `feats` already ARE encoder outputs [n, T, d]: exercises adaptor + splice at full width without
        paying for an encoder"""

        def __init__(self):
            super().__init__(modality="audio", is_discrete=False)

        def feature_dim(self):
            return d_model

        def copy_for_worker(self):
            return self

        def encode_batch(self, feats, lengths):
            return [f[: int(n)] for f, n in zip(feats, lengths)]

    return _Cont()


def wide_llm_cfg(n_layers=2):
    cfg = dict(oracle.qwen2.config_7b())
    cfg["num_hidden_layers"] = n_layers
    return cfg


def wide_enc_cfg():
    cfg = dict(oracle.afwhisper.default_config())
    cfg["encoder_layers"] = 1
    return cfg


def build_wide_llm(n_layers=2, dtype=torch.bfloat16, device="cuda:0", seed=3, d_enc=1280, real_audio=False, enc_seed=4):
    """(model on the GPU, f32 CPU state dict holding the SAME values the model computes with, cfg, vocab, intervals).
    Weights come from the per-tensor seeded generator, are rounded to `dtype` once, and both sides start from the rounded
    values -- so the only difference left between HIP and oracle is the arithmetic.
    real_audio: the continuous IO is the real ContinuousAudioIO over a full-width ONE-layer AF-Whisper encoder (the
    configuration oracle/make_golden_7b.py captured from the reference) instead of the pass-through stub; the returned model
    then carries the preprocessor as `model._test_pre` and the encoder state dict as `model._test_enc_sd`."""
    from audio_intelligence_amd.lm.parallel import ParallelLLM
    from audio_intelligence_amd import ualm_job
    cfg = wide_llm_cfg(n_layers)
    text_io, audio_io = stub_ios(cfg["text_vocab"])
    enc_sd = None
    if real_audio:
        from audio_intelligence_amd.multimodal_io.audio import ContinuousAudioIO
        from audio_intelligence_amd.multimodal_io.modeling_whisper import AFWhisperEncoder, AFWhisperEncoderConfig
        ecfg = wide_enc_cfg()
        enc_sd = {k: v.to(dtype) for k, v in syn.synth_state_dict(syn.encoder_param_shapes(ecfg), enc_seed).items()}
        enc = AFWhisperEncoder(AFWhisperEncoderConfig.from_dict(ecfg))
        enc.load_state_dict(enc_sd, strict=True)
        cont = ContinuousAudioIO(encoder_choice="AFWhisper", dtype=str(dtype).replace("torch.", ""), device=device, encoder=enc)
        enc_sd = {k: v.float() for k, v in enc_sd.items()}
    else:
        cont = stub_continuous(d_enc)
    ios = {"text": text_io, "discrete_audio": audio_io, "continuous_audio": cont}
    vocab, iv = ualm_job.build_vocabulary(ios)
    hf = {"architectures": ["Qwen2ForCausalLM"], "hidden_size": cfg["hidden_size"], "num_hidden_layers": n_layers,
          "num_attention_heads": cfg["num_attention_heads"], "num_key_value_heads": cfg["num_key_value_heads"],
          "intermediate_size": cfg["intermediate_size"], "rope_theta": cfg["rope_theta"], "rms_norm_eps": cfg["rms_norm_eps"],
          "vocab_size": cfg["text_vocab"]}
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.device(device):
            model = ParallelLLM(hf, ios, vocab, iv)
    finally:
        torch.set_default_dtype(old)
    sd = {}
    with torch.no_grad():
        params = dict(model.named_parameters())
        for name, shape in syn.llm_param_shapes(cfg, len(vocab), 8, d_enc):
            t = syn.synth_tensor(name, shape, seed).to(dtype)
            params[name].copy_(t)
            sd[name] = t.float()
    model.prepare_inference()
    model.eval()
    if real_audio:
        model._test_pre = ualm_job.UALMPreprocessor(False, {k: v.copy_for_worker() for k, v in ios.items()}, vocab, iv)
        model._test_enc_sd = enc_sd
    return model, sd, cfg, vocab, iv


# the LLM widths the float64 reference tests run at: (H, inter, n_q, n_kv)
LLM_WIDTHS = [(512, 4096, 8, 2), (1024, 4096, 8, 1), (1536, 8704, 12, 2), (2048, 5632, 32, 4), (4096, 4096, 64, 32), (1536, 8960, 12, 2),
              (896, 4864, 14, 2)]


def llm_cfg_at(Hd, I, nq, nkv):
    """the 2-layer Qwen2 config of build_llm_at at one width"""
    return dict(hidden_size=Hd, num_hidden_layers=2, num_attention_heads=nq, num_key_value_heads=nkv, intermediate_size=I,
                rope_theta=1e6, rms_norm_eps=1e-6)


def llm_weights_f64(cfg, vocab=2048, seed=3, dtype=torch.bfloat16):
    """build_llm_at's weights on the CPU (synthetic.synth_tensor, rounded to `dtype` once), held as float64; the LLM's tensors only"""
    return {n: syn.synth_tensor(n, s, seed).to(dtype).to(torch.float64)
            for n, s in syn.llm_param_shapes(cfg, vocab, 8, 8) if not n.startswith(("adaptor", "stream"))}


def build_llm_at(shape, text_vocab, seed=3, dtype=torch.bfloat16, device="cuda:0"):
    """build_wide_llm's recipe at `shape` = (H, inter, n_q, n_kv), 2 layers, a `text_vocab`-id text vocabulary: (model on the GPU,
    float64 CPU state dict of the same `dtype` values (the LLM's tensors only), cfg)"""
    from audio_intelligence_amd.lm.parallel import ParallelLLM
    from audio_intelligence_amd import ualm_job
    Hd, I, nq, nkv = shape
    cfg = dict(hidden_size=Hd, num_hidden_layers=2, num_attention_heads=nq, num_key_value_heads=nkv, intermediate_size=I,
               rope_theta=1e6, rms_norm_eps=1e-6, text_vocab=text_vocab)
    text_io, audio_io = stub_ios(text_vocab)
    ios = {"text": text_io, "discrete_audio": audio_io, "continuous_audio": stub_continuous(64)}
    vocab, iv = ualm_job.build_vocabulary(ios)
    hf = {"architectures": ["Qwen2ForCausalLM"], "hidden_size": Hd, "num_hidden_layers": 2, "num_attention_heads": nq,
          "num_key_value_heads": nkv, "intermediate_size": I, "rope_theta": 1e6, "rms_norm_eps": 1e-6, "vocab_size": text_vocab}
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.device(device):
            model = ParallelLLM(hf, ios, vocab, iv)
    finally:
        torch.set_default_dtype(old)
    sd = {}
    with torch.no_grad():
        params = dict(model.named_parameters())
        for name, shp in syn.llm_param_shapes(cfg, len(vocab), 8, 64):
            t = syn.synth_tensor(name, shp, seed).to(dtype)
            params[name].copy_(t)
            if not name.startswith(("adaptor", "stream")):
                sd[name] = t.to(torch.float64)
    model.prepare_inference()
    model.eval()
    return model, sd, cfg
