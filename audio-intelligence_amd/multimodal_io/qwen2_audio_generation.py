"""AF3 / Qwen2-Audio style `generate()` surface over the HIP kernels.

Host-side mirror of `Qwen2AudioForConditionalGeneration` (UALM/models/ualm/multimodal_io/modeling_whisper.py:855-1369): same
sub-module names (`audio_tower`, `multi_modal_projector`, `language_model`), hence the same state-dict keys; same `forward`
arguments and return fields (`logits`, `past_key_values`, `attention_mask`); `prepare_inputs_for_generation` with the reference's
three input-slicing rules (:1250-1318); a greedy `generate()`.  `<|AUDIO|>` placeholders are widened by the merge that is already
pinned to the reference (`merge_input_ids_with_audio_features`, :913-1108).

Padded batches without a padding mask in the kernels: the merged batch is COMPACTED -- each sequence's valid tokens are moved to
cache slots [0, len_b) -- which is exactly what the reference's `attention_mask` + `position_ids = cumsum(mask) - 1` compute
(pad keys are never attended, valid tokens get positions 0 .. len_b - 1), for left- and right-padded batches alike.  Prefill then
runs as one causal batch over [B, max len] (rows past len_b are dead: nothing valid attends to them and decode overwrites their
cache slots), and each decode step appends at the per-sequence slot `seq_len[b]` through `afhip_llm_forward_ragged`.
"""
import ctypes as C
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from .modeling_whisper import (AFWhisperEncoder, AFWhisperEncoderConfig, Qwen2AudioMultiModalProjector, _Linear,
                               merge_input_ids_with_audio_features)


def _get(cfg, name, default=None):
    return cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)


# GenerationConfig fields this generate() serves; every other processor / search knob raises NotImplementedError when set to a
# non-neutral value (the neutral values are those under which GenerationMixin._get_logits_processor adds nothing)
_SERVED = ("max_new_tokens", "max_length", "eos_token_id", "pad_token_id", "do_sample", "temperature", "top_k", "top_p",
           "repetition_penalty", "return_dict_in_generate", "output_scores", "output_logits")
_SET = lambda v: v is not None
_UNSERVED = {
    "min_p": _SET, "top_h": _SET, "typical_p": lambda v: v is not None and v < 1.0,
    "epsilon_cutoff": lambda v: v is not None and 0.0 < v < 1.0, "eta_cutoff": lambda v: v is not None and 0.0 < v < 1.0,
    "num_beams": lambda v: v is not None and v > 1, "num_beam_groups": lambda v: v is not None and v > 1,
    "num_return_sequences": lambda v: v is not None and v > 1, "diversity_penalty": lambda v: v is not None and v != 0.0,
    "penalty_alpha": lambda v: v is not None and v > 0, "no_repeat_ngram_size": lambda v: v is not None and v > 0,
    "encoder_no_repeat_ngram_size": lambda v: v is not None and v > 0,
    "encoder_repetition_penalty": lambda v: v is not None and v != 1.0, "bad_words_ids": _SET, "force_words_ids": _SET,
    "constraints": _SET, "min_length": lambda v: v is not None and v > 0, "min_new_tokens": lambda v: v is not None and v > 0,
    "sequence_bias": _SET, "suppress_tokens": _SET, "begin_suppress_tokens": _SET, "forced_bos_token_id": _SET,
    "forced_eos_token_id": _SET, "exponential_decay_length_penalty": _SET, "guidance_scale": lambda v: v is not None and v != 1,
    "renormalize_logits": lambda v: v is True, "remove_invalid_values": lambda v: v is True, "watermarking_config": _SET,
    "stop_strings": _SET, "max_time": _SET, "output_attentions": lambda v: v is True, "output_hidden_states": lambda v: v is True,
    "logits_processor": lambda v: v is not None and len(v) > 0, "stopping_criteria": lambda v: v is not None and len(v) > 0,
    "prefix_allowed_tokens_fn": _SET, "assistant_model": _SET, "streamer": _SET, "prompt_lookup_num_tokens": _SET,
    "dola_layers": _SET, "token_healing": lambda v: v is True,
}
_IGNORED = ("use_cache", "bos_token_id", "decoder_start_token_id", "early_stopping", "length_penalty", "cache_implementation",
            "transformers_version", "synced_gpus")


def _generation_knobs(generation_config, kwargs, **explicit) -> dict:
    """GenerationConfig / dict + explicit arguments (which win) -> the served knobs; unserved knobs that are set raise."""
    if generation_config is None:
        base = {}
    elif isinstance(generation_config, dict):
        base = dict(generation_config)
    elif hasattr(generation_config, "to_dict"):
        base = generation_config.to_dict()
    else:
        base = dict(vars(generation_config))
    for name, v in kwargs.items():
        if name not in _UNSERVED and name not in _IGNORED:
            raise TypeError(f"generate() got an unexpected keyword argument '{name}'")
    merged = {**base, **kwargs}
    for name, is_set in _UNSERVED.items():
        if name in merged and is_set(merged[name]):
            raise NotImplementedError(f"generate(): `{name}`={merged[name]!r} is not supported (served: {', '.join(_SERVED)})")
    out = {n: base.get(n) for n in _SERVED}
    out.update({n: v for n, v in explicit.items() if v is not None})
    return out


# beam-search knobs (GenerationMixin._beam_search) and the values under which they ask for nothing
_BEAM_NEUTRAL = {"num_beams": 1, "num_return_sequences": 1, "length_penalty": 1.0, "early_stopping": False}


def _beam_knobs(generation_config, kwargs, do_sample=None):
    """Peels the beam-search knobs off `kwargs` / `generation_config` (explicit kwargs win).  Returns (beam, generation_config,
    kwargs): `beam` is None -- and the inputs come back unchanged, so `_generation_knobs` judges them as before -- unless
    num_beams > 1 without sampling; then `beam` holds num_beams / num_return_sequences / length_penalty / early_stopping and the
    returned config and kwargs carry the neutral values of those four."""
    if generation_config is None:
        base = {}
    elif isinstance(generation_config, dict):
        base = dict(generation_config)
    elif hasattr(generation_config, "to_dict"):
        base = generation_config.to_dict()
    else:
        base = dict(vars(generation_config))
    merged = {**base, **{k: v for k, v in kwargs.items() if k in _BEAM_NEUTRAL}}
    nb = merged.get("num_beams")
    sampling = do_sample if do_sample is not None else kwargs.get("do_sample", base.get("do_sample"))
    if nb is None or nb <= 1 or sampling:
        return None, generation_config, kwargs
    beam = {k: (merged[k] if merged.get(k) is not None else v) for k, v in _BEAM_NEUTRAL.items()}
    beam["num_beams"] = int(nb)
    beam["num_return_sequences"] = int(beam["num_return_sequences"])
    beam["length_penalty"] = float(beam["length_penalty"])
    if beam["early_stopping"] not in (True, False, "never"):
        raise ValueError(f"`early_stopping` must be True, False or 'never', got {beam['early_stopping']!r}")
    if beam["num_return_sequences"] > beam["num_beams"]:
        raise ValueError("`num_return_sequences` has to be smaller or equal to `num_beams`.")
    return beam, {**base, **_BEAM_NEUTRAL}, {k: v for k, v in kwargs.items() if k not in _BEAM_NEUTRAL}


def _gather_beams(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """t [B, n, ...], idx [B, k] -> t[b, idx[b, j], ...] (GenerationMixin._gather_beams)"""
    return torch.take_along_dim(t, idx.view(idx.shape + (1,) * (t.dim() - 2)), dim=1)


class _CausalLM(nn.Module):
    """`Qwen2ForCausalLM` parameter layout: `model.embed_tokens / layers / norm` + `lm_head` (no bias)."""

    def __init__(self, text_config: dict):
        super().__init__()
        from ..lm.parallel import _Backbone
        self.cfg = dict(text_config)
        self.model = _Backbone(self.cfg, self.cfg["vocab_size"])
        self.lm_head = _Linear(self.cfg["hidden_size"], self.cfg["vocab_size"], bias=False)
        self._packed = None

    def _apply(self, fn, *a, **kw):
        self._packed = None
        return super()._apply(fn, *a, **kw)

    def _load_from_state_dict(self, *a, **kw):
        self._packed = None
        return super()._load_from_state_dict(*a, **kw)

    def pack(self, max_positions=None):
        from ..lm.parallel import pack_qwen2_weights
        if self._packed is None or (max_positions is not None and max_positions > self._packed.max_pos):
            self._packed = pack_qwen2_weights(self.model, self.lm_head.weight, None, self.cfg, 1, max_positions=max_positions)
        return self._packed


class AF3Cache:
    """KV cache of a (possibly ragged) batch in compact layout + the bookkeeping `generate()` needs.  `get_seq_length()` is the
    length of the PADDED layout the caller sees (merged prompt width + generated tokens), like the reference's cache."""

    def __init__(self, kv, seq_len: torch.Tensor, padded_len: int, compact_len: int):
        self.kv, self.seq_len, self.padded_len = kv, seq_len, padded_len
        self.compact_len = compact_len            # longest sequence in cache slots (host-side bound for capacity checks)
        self.seen_tokens = padded_len

    def get_seq_length(self):
        return self.padded_len


class Qwen2AudioForConditionalGeneration(nn.Module):
    def __init__(self, config):
        """config: `audio_config` (fields of Qwen2AudioEncoderConfig), `text_config` (Qwen2 config dict: hidden_size,
        num_hidden_layers, num_attention_heads, num_key_value_heads, intermediate_size, vocab_size, rope_theta, rms_norm_eps),
        `audio_token_index`, optional `pad_token_id`, `ignore_index` (-100), `eos_token_id`."""
        super().__init__()
        self.config = config if not isinstance(config, dict) else SimpleNamespace(**config)
        acfg, tcfg = _get(config, "audio_config"), _get(config, "text_config")
        acfg = acfg if isinstance(acfg, dict) else vars(acfg)
        tcfg = tcfg if isinstance(tcfg, dict) else vars(tcfg)
        self.audio_tower = AFWhisperEncoder(AFWhisperEncoderConfig.from_dict(acfg))
        self.multi_modal_projector = Qwen2AudioMultiModalProjector(d_model=self.audio_tower.config.d_model, hidden_size=tcfg["hidden_size"])
        self.vocab_size = tcfg["vocab_size"]
        self.language_model = _CausalLM(tcfg)
        pad = _get(config, "pad_token_id")
        self.pad_token_id = pad if pad is not None else -1
        self.audio_token_index = _get(config, "audio_token_index")
        self.ignore_index = _get(config, "ignore_index", -100)
        self._padding_side = "left"
        self._ws = None

    # ---- modeling_whisper.py:866-875
    @property
    def padding_side(self):
        return self._padding_side

    @padding_side.setter
    def padding_side(self, padding_side: str):
        if padding_side not in ["left", "right"]:
            raise ValueError(f"{padding_side} is not `left` or `right`.")
        self._padding_side = padding_side

    @property
    def dtype(self):
        return self.language_model.lm_head.weight.dtype

    @property
    def device(self):
        return self.language_model.lm_head.weight.device

    def get_input_embeddings(self):
        table = self.language_model.model.embed_tokens.weight
        return lambda ids: ops.embed_sum(ids.to(table.device).unsqueeze(-1), table)

    def get_output_embeddings(self):
        return self.language_model.lm_head

    def _merge_input_ids_with_audio_features(self, audio_features, num_audio_tokens, inputs_embeds, input_ids, attention_mask, labels):
        return merge_input_ids_with_audio_features(audio_features, num_audio_tokens, inputs_embeds, input_ids, attention_mask, labels,
                                                   audio_token_index=self.audio_token_index, pad_token_id=self.pad_token_id,
                                                   ignore_index=self.ignore_index, padding_side=self.padding_side)

    # ---- device plumbing
    def _workspace(self, B, T, max_ctx):
        lib = L.lib()
        need = lib.afhip_llm_workspace_bytes(C.byref(self.language_model.pack().w), B, T, max_ctx)
        if self._ws is None or self._ws.numel() < need or self._ws.device != self.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _new_kv(self, B, cap):
        from ..lm.parallel import KVCache
        pk = self.language_model.pack(cap)
        return KVCache(self.language_model.cfg["num_hidden_layers"], B, pk.nkv, (cap + 63) // 64 * 64, pk.hd, self.dtype, self.device)

    def _head(self, hidden_rows: torch.Tensor) -> torch.Tensor:
        """[n, H] final-normed rows -> [n, V] f32 logits."""
        lib = L.lib()
        hidden_rows = hidden_rows.contiguous()
        n = hidden_rows.shape[0]
        ws = torch.empty(n * hidden_rows.shape[1] * hidden_rows.element_size() + 256, dtype=torch.uint8, device=hidden_rows.device)
        return torch.ops.afhip.lm_head(self.language_model.pack().blob, hidden_rows, 1, ws)[:, 0]

    def _encode_audio(self, input_features, feature_attention_mask):
        """modeling_whisper.py:1181-1207: per-clip key length from the feature mask, encoder, projector."""
        tower = self.audio_tower
        audio_feat_lengths, audio_output_lengths = tower._get_feat_extract_output_lengths(feature_attention_mask.sum(-1))
        x = input_features.to(self.device)
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        mel_btc = ops.transpose_cast(x.contiguous(), tower.dtype)
        feats = tower.encode_btc(mel_btc, feat_len=audio_feat_lengths.clamp(max=tower.config.max_source_positions))
        return self.multi_modal_projector(feats), audio_output_lengths

    # ---- forward (modeling_whisper.py:1112-1248)
    @torch.no_grad()
    def forward(self, input_ids=None, input_features=None, attention_mask=None, feature_attention_mask=None, position_ids=None,
                past_key_values: Optional[AF3Cache] = None, inputs_embeds=None, labels=None, use_cache=None, output_attentions=None,
                output_hidden_states=None, return_dict=None, logits_to_keep: int = 0, max_new_tokens: int = 64):
        """Returns a namespace with `logits` [B, L', V] (model dtype; rows of padding positions are zero -- the reference computes
        unspecified values there), `past_key_values`, `attention_mask` (the merged one, as the reference's output carries it).
        `logits_to_keep` = k > 0 restricts the head to the last k positions of the padded layout (0 = all, the reference's
        behaviour); `max_new_tokens` only sizes the cache it creates.  `labels` are carried through the merge; no loss (inference
        path).  `position_ids` is accepted for signature parity: positions are cumsum(mask) - 1, which is what the reference
        computes for generation (:1293-1299)."""
        if output_attentions or output_hidden_states:
            raise NotImplementedError("output_attentions / output_hidden_states are not available from the fused kernels")
        lib = L.lib()
        dev = self.device
        if past_key_values is not None:
            # ---- one new token per sequence against the cache
            if inputs_embeds is None:
                if input_ids.shape[1] != 1:
                    raise ValueError("with past_key_values, pass exactly one new token per sequence")
                inputs_embeds = self.get_input_embeddings()(input_ids.to(dev))
            c = past_key_values
            B = inputs_embeds.shape[0]
            if c.compact_len + 1 > c.kv.cap:
                raise L.AfhipError(f"KV cache capacity {c.kv.cap} exhausted: create the cache with a larger max_new_tokens")
            max_pos = c.kv.cap - 1
            pk = self.language_model.pack(c.kv.cap)
            x = inputs_embeds.reshape(B, -1).to(self.dtype).contiguous()
            ws = self._workspace(B, 1, c.kv.cap)
            hid = torch.ops.afhip.llm_forward_ragged(pk.blob, x, c.seq_len, max_pos, c.kv.k, c.kv.v, ws)
            c.seq_len += 1
            c.padded_len += 1
            c.compact_len += 1
            c.seen_tokens = c.padded_len
            logits = self._head(hid).to(self.dtype).view(B, 1, -1)
            if attention_mask is not None:
                attention_mask = attention_mask.to(dev)
            return SimpleNamespace(loss=None, logits=logits, past_key_values=c, hidden_states=None, attentions=None, attention_mask=attention_mask)

        # ---- prompt
        hid, cache, mask, attention_mask, labels, position_ids = self._prefill(input_ids, input_features, attention_mask, feature_attention_mask,
                                                                               inputs_embeds, labels, max_new_tokens)
        B, Lp = mask.shape
        # logits back in the padded layout
        keep = Lp if logits_to_keep in (0, None) else min(int(logits_to_keep), Lp)
        cols = torch.arange(Lp - keep, Lp, device=dev)
        rank = torch.cumsum(mask.long(), dim=1) - 1                                       # compact slot of every valid padded position
        sel_valid = mask[:, cols]
        rows = hid[torch.arange(B, device=dev)[:, None].expand(B, keep)[sel_valid], rank[:, cols][sel_valid]]
        logits = torch.zeros((B, keep, self.vocab_size), dtype=self.dtype, device=dev)
        if rows.shape[0] > 0:
            logits[sel_valid] = self._head(rows).to(self.dtype)
        return SimpleNamespace(loss=None, logits=logits, past_key_values=cache if use_cache is not False else None, hidden_states=None,
                               attentions=None, attention_mask=attention_mask, labels=labels, position_ids=position_ids)

    def _prefill(self, input_ids, input_features, attention_mask, feature_attention_mask, inputs_embeds, labels, max_new_tokens):
        """embed -> (audio tower -> projector -> merge) -> compact -> causal prefill.  Returns the compact final-normed hidden
        states [B, max len, H], the cache, the boolean merged mask [B, L'], and the merge's other outputs."""
        lib = L.lib()
        dev = self.device
        position_ids = None
        if inputs_embeds is None:
            input_ids = input_ids.to(dev)
            inputs_embeds = self.get_input_embeddings()(input_ids)
            if attention_mask is None:
                attention_mask = torch.ones_like(input_ids)
            attention_mask = attention_mask.to(dev)
            if input_features is not None and input_ids.shape[1] != 1:
                audio_features, audio_output_lengths = self._encode_audio(input_features, feature_attention_mask.to(dev))
                inputs_embeds, attention_mask, labels, position_ids, _ = self._merge_input_ids_with_audio_features(
                    audio_features, audio_output_lengths, inputs_embeds, input_ids, attention_mask, labels)
        elif attention_mask is None:
            attention_mask = torch.ones(inputs_embeds.shape[:2], dtype=torch.long, device=dev)
        B, Lp, H = inputs_embeds.shape
        mask = attention_mask.to(dev).bool()
        lens = mask.sum(-1)
        Lmax = int(lens.max())
        # compact layout: valid tokens of sequence b -> slots [0, len_b) (stable order)
        order = torch.argsort((~mask).to(torch.int8), dim=1, stable=True)               # valid positions first, original order kept
        xc = torch.gather(inputs_embeds.to(self.dtype), 1, order[:, :Lmax, None].expand(B, Lmax, H)).contiguous()
        kv = self._new_kv(B, Lmax + max_new_tokens + 1)
        pk = self.language_model.pack(kv.cap)
        ws = self._workspace(B, Lmax, kv.cap)
        hid = torch.ops.afhip.llm_forward(pk.blob, xc, 0, kv.k, kv.v, ws)
        kv.length = Lmax
        return hid, AF3Cache(kv, lens.to(torch.int32).contiguous(), Lp, Lmax), mask, attention_mask, labels, position_ids

    __call__ = forward

    # ---- modeling_whisper.py:1250-1318
    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, inputs_embeds=None, input_features=None, attention_mask=None, **kwargs):
        if past_key_values is not None:
            cache_length = past_length = past_key_values.get_seq_length()
            if input_features is not None and kwargs.get("attention_mask") is not None:
                attention_mask = kwargs["attention_mask"]
                attention_mask = torch.cat([attention_mask, attention_mask.new_ones((attention_mask.shape[0], 1))], dim=-1)
            if attention_mask is not None and attention_mask.shape[1] > input_ids.shape[1]:
                input_ids = input_ids[:, -(attention_mask.shape[1] - past_length):]
            elif past_length < input_ids.shape[1]:
                input_ids = input_ids[:, past_length:]
            elif self.audio_token_index in input_ids:
                input_ids = input_ids[:, input_ids.shape[1] - 1:]
            if cache_length < past_length and attention_mask is not None:
                attention_mask = attention_mask[:, -(cache_length + input_ids.shape[1]):]
        position_ids = kwargs.get("position_ids", None)
        if attention_mask is not None and position_ids is None:
            position_ids = attention_mask.long().cumsum(-1) - 1
            position_ids.masked_fill_(attention_mask == 0, 1)
            if past_key_values:
                position_ids = position_ids[:, -input_ids.shape[1]:]
        if inputs_embeds is not None and past_key_values is None:
            model_inputs = {"inputs_embeds": inputs_embeds}
        else:
            model_inputs = {"input_ids": input_ids}
        model_inputs.update({"position_ids": position_ids, "past_key_values": past_key_values, "use_cache": kwargs.get("use_cache"),
                             "attention_mask": attention_mask, "input_features": input_features,
                             "feature_attention_mask": kwargs.get("feature_attention_mask", None)})
        return model_inputs

    # ---- generation (GenerationMixin.generate: greedy and multinomial sampling)
    @torch.no_grad()
    def generate(self, input_ids, input_features=None, attention_mask=None, feature_attention_mask=None, max_new_tokens: Optional[int] = None,
                 eos_token_id=None, pad_token_id=None, do_sample: Optional[bool] = None, temperature: Optional[float] = None,
                 top_k: Optional[int] = None, top_p: Optional[float] = None, repetition_penalty: Optional[float] = None,
                 generation_config=None, return_dict_in_generate: Optional[bool] = None, output_scores: Optional[bool] = None,
                 output_logits: Optional[bool] = None, generator: Optional[torch.Generator] = None, **kwargs):
        """Returns [B, L + n_new] = the prompt ids followed by the generated ones; a sequence that has emitted `eos_token_id` is continued
        with `pad_token_id` (HF semantics), generation stops when every sequence has finished.

        HF knobs, with GenerationMixin's semantics: `do_sample`, `temperature`, `top_k`, `top_p`, `repetition_penalty`, `max_length`,
        taken from `generation_config` (a GenerationConfig or a dict) unless passed explicitly.  An unset or neutral knob applies no
        processor (top_k None / 0, top_p >= 1, temperature None / 1, repetition_penalty None / 1); any other processor knob that is
        set raises NotImplementedError.  The processors and the draw run in one HIP kernel (afhip_sample_filter); the draw takes one
        `torch.rand(B, generator=generator)` per step (`generator` is an extension: a fixed seed gives a fixed token stream).
        `return_dict_in_generate=True` returns a namespace with `sequences`, and `scores` (processed rows, `output_scores`) / `logits`
        (raw rows, `output_logits`) as tuples of [B, V] f32 per step.

        Beam search (GenerationMixin._beam_search): `num_beams` > 1 without sampling, with `num_return_sequences` (<= num_beams),
        `length_penalty` and `early_stopping` (True, False, "never"); see `_generate_beam`.  Beam sampling and a repetition
        penalty under beams raise NotImplementedError."""
        beam, generation_config, kwargs = _beam_knobs(generation_config, kwargs, do_sample)
        cfg = _generation_knobs(generation_config, kwargs, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
                                do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty,
                                return_dict_in_generate=return_dict_in_generate, output_scores=output_scores, output_logits=output_logits)
        max_new = cfg.get("max_new_tokens")
        if max_new is None:
            max_new = cfg["max_length"] - input_ids.shape[1] if cfg.get("max_length") is not None else 20
        rp = cfg.get("repetition_penalty")
        if beam is not None:
            if rp not in (None, 1.0):
                raise NotImplementedError("generate(): `repetition_penalty` is not supported with num_beams > 1")
            return self._generate_beam(input_ids, input_features, attention_mask, feature_attention_mask, max_new, cfg, beam)
        sampling = bool(cfg.get("do_sample"))
        want_dict = bool(cfg.get("return_dict_in_generate"))
        if not sampling and rp in (None, 1.0) and not want_dict:
            return self._generate_greedy(input_ids, input_features, attention_mask, feature_attention_mask, max_new,
                                         cfg.get("eos_token_id"), cfg.get("pad_token_id"))
        return self._generate_filtered(input_ids, input_features, attention_mask, feature_attention_mask, max_new, cfg, generator)

    def _eos_pad(self, eos_token_id, pad_token_id):
        eos = eos_token_id if eos_token_id is not None else _get(self.config, "eos_token_id")
        eos = [] if eos is None else ([eos] if isinstance(eos, int) else list(eos))
        pad = pad_token_id if pad_token_id is not None else (self.pad_token_id if self.pad_token_id >= 0 else (eos[0] if eos else 0))
        return eos, pad

    @torch.no_grad()
    def _generate_filtered(self, input_ids, input_features, attention_mask, feature_attention_mask, max_new_tokens, cfg, generator):
        """Greedy with a repetition penalty, or multinomial sampling: every step's logits go through afhip_sample_filter."""
        dev = self.device
        eos, pad = self._eos_pad(cfg.get("eos_token_id"), cfg.get("pad_token_id"))
        sampling = bool(cfg.get("do_sample"))
        V = self.vocab_size
        T = cfg.get("temperature") if sampling else None
        T = 1.0 if T is None else float(T)
        if not T > 0:
            raise ValueError(f"`temperature` (={T}) has to be a strictly positive float")
        k = cfg.get("top_k") if sampling else None
        k = 0 if k is None else int(k)
        if k < 0:
            raise ValueError(f"`top_k` has to be a strictly positive integer, but is {k}")
        p = cfg.get("top_p") if sampling else None
        p = 1.0 if p is None or p >= 1.0 else float(p)
        if p < 0:
            raise ValueError(f"`top_p` has to be a float >= 0 and <= 1, but is {p}")
        p = max(p, 2.0 ** -40)                                   # top_p = 0 keeps the top value (min_tokens_to_keep = 1)
        rp = cfg.get("repetition_penalty")
        rp = 1.0 if rp is None else float(rp)
        if not rp > 0:
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {rp}")
        out_scores, out_logits = bool(cfg.get("output_scores")), bool(cfg.get("output_logits"))
        input_ids = input_ids.to(dev)
        hid, cache, mask, _, _, _ = self._prefill(input_ids, input_features, attention_mask, feature_attention_mask, None, None, max_new_tokens)
        B, W = input_ids.shape
        nxt_logits = self._head(hid[torch.arange(B, device=dev), cache.seq_len.long() - 1]).to(self.dtype)
        pen_ids = n_ids = None
        if rp != 1.0:
            # what RepetitionPenaltyLogitsProcessor sees: the caller's ids (pads and <|AUDIO|> placeholders included), then the
            # generated ones -- a device buffer appended to in place, never rebuilt on the host
            pen_ids = torch.empty((B, W + max_new_tokens), dtype=torch.int32, device=dev)
            pen_ids[:, :W] = input_ids
            n_ids = torch.full((B,), W, dtype=torch.int32, device=dev)
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        new, scores, raw = [], [], []
        for step in range(max_new_tokens):
            lg = nxt_logits.float().contiguous()
            if out_logits:
                raw.append(lg)
            sc = torch.empty((B, V), dtype=torch.float32, device=dev) if out_scores else None
            u = torch.rand(B, generator=generator, device=dev) if sampling else None
            tok = ops.sample_filter(lg, temperature=T, top_k=min(k, V), top_p=p, penalty=rp, penalty_ids=pen_ids, n_ids=n_ids, u=u, scores=sc)
            if out_scores:
                scores.append(sc)
            tok = torch.where(unfinished, tok, torch.full_like(tok, pad))
            new.append(tok)
            if pen_ids is not None:
                pen_ids[:, W + step] = tok.to(torch.int32)
                n_ids += 1
            for e in eos:
                unfinished = unfinished & (tok != e)
            if not bool(unfinished.any()) or step == max_new_tokens - 1:
                break
            o = self.forward(input_ids=tok[:, None], past_key_values=cache, use_cache=True)
            nxt_logits, cache = o.logits[:, -1], o.past_key_values
        seqs = torch.cat([input_ids, torch.stack(new, dim=1)], dim=1)
        if not cfg.get("return_dict_in_generate"):
            return seqs
        return SimpleNamespace(sequences=seqs, scores=tuple(scores) if out_scores else None, logits=tuple(raw) if out_logits else None,
                               attentions=None, hidden_states=None, past_key_values=None)

    @torch.no_grad()
    def _generate_beam(self, input_ids, input_features, attention_mask, feature_attention_mask, max_new_tokens, cfg, beam):
        """Beam search with GenerationMixin._beam_search's semantics (steps b-g, finalisation and cropping).  The audio tower and the
        prefill run once for the B prompts; the cache is then expanded to B * num_beams slots by afhip_kv_gather.  Per step,
        afhip_beam_select picks the top max(2, 1 + n_eos) * num_beams continuations of each prompt, HF's bookkeeping runs as small
        device tensor ops, afhip_kv_gather reorders the generated rows of the cache in place, and the ragged decode feeds the selected
        tokens.  The prompt width W of `input_ids` is HF's decoder_prompt_len: max_length = W + max_new_tokens."""
        from ..lm.parallel import KVCache
        lib = L.lib()
        dev = self.device
        nb, nrs, lp, es = beam["num_beams"], beam["num_return_sequences"], beam["length_penalty"], beam["early_stopping"]
        if max_new_tokens < 1:
            raise ValueError("beam search needs max_new_tokens >= 1")
        eos, pad = self._eos_pad(cfg.get("eos_token_id"), cfg.get("pad_token_id"))
        out_scores, out_logits = bool(cfg.get("output_scores")), bool(cfg.get("output_logits"))
        V = self.vocab_size
        input_ids = input_ids.to(dev)
        B, W = input_ids.shape
        R = B * nb
        max_length = W + max_new_tokens
        hid, cache0, _, _, _, _ = self._prefill(input_ids, input_features, attention_mask, feature_attention_mask, None, None, max_new_tokens)
        lens = cache0.seq_len
        nxt_logits = self._head(hid[torch.arange(B, device=dev), lens.long() - 1]).to(self.dtype).repeat_interleave(nb, 0)
        del hid
        # B prompts -> R = B * nb slots: slot r takes the prompt rows of prompt r // nb
        k0 = cache0.kv
        kv = KVCache(k0.k.shape[0], R, k0.k.shape[2], k0.cap, k0.k.shape[4], self.dtype, dev)
        row0 = lens.repeat_interleave(nb).contiguous()                       # prompt length of every slot: generated rows start here
        ops.kv_gather(k0.k, k0.v, kv.k, kv.v, (torch.arange(R, device=dev, dtype=torch.int32) // nb).contiguous(),
                      torch.zeros(R, dtype=torch.int32, device=dev), row0, cache0.compact_len)
        kv.length = k0.length
        cache = AF3Cache(kv, row0.clone(), cache0.padded_len, cache0.compact_len)
        del cache0, k0
        kv_ws = torch.empty(max(lib.afhip_kv_gather_workspace_bytes(kv.k.shape[0], R, kv.k.shape[2], kv.k.shape[4], max_new_tokens,
                                                                    L.dtype_code(self.dtype)), 1), dtype=torch.uint8, device=dev)

        K = max(2, 1 + len(eos)) * nb
        top_nb = torch.arange(K, device=dev) < nb
        eos_t = torch.tensor(eos, dtype=torch.int64, device=dev)
        fill = (pad if pad else eos[0]) if eos else -1                       # transformers: `pad or eos[0]`, -1 without an eos
        running_seq = torch.full((B, nb, max_length), fill, dtype=torch.int64, device=dev)
        running_seq[:, :, :W] = input_ids[:, None]
        sequences = running_seq.clone()
        running_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
        running_scores[:, 1:] = -1e9
        beam_scores = torch.full((B, nb), -1e9, dtype=torch.float32, device=dev)
        finished = torch.zeros((B, nb), dtype=torch.bool, device=dev)
        improvable = torch.ones((B, 1), dtype=torch.bool, device=dev)
        running_bi = torch.full((B, nb, max_length - W), -1, dtype=torch.int32, device=dev)
        beam_indices = running_bi.clone()
        offs = torch.arange(B, device=dev)[:, None] * nb
        scores, raw = [], []
        cur_len = W
        while True:
            lg = nxt_logits.float().contiguous()
            if out_logits:
                raw.append(lg)
            sc = torch.empty((R, V), dtype=torch.float32, device=dev) if out_scores else None
            topv, topi = ops.beam_select(lg, running_scores, K, model_dtype=self.dtype, scores=sc)
            if out_scores:
                scores.append(sc)
            # c. continuations
            src_beam = topi // V
            topk_seq = _gather_beams(running_seq, src_beam)
            topk_seq[:, :, cur_len] = topi % V
            topk_bi = _gather_beams(running_bi, src_beam)
            topk_bi[:, :, cur_len - W] = (src_beam + offs).to(torch.int32)
            # d. stopping criteria: an eos id, or max_length
            hits = torch.isin(topk_seq[:, :, cur_len], eos_t) if eos else torch.zeros_like(top_nb[None].expand(B, K))
            if cur_len + 1 >= max_length:
                hits = torch.ones_like(hits)
            # e. the best num_beams unfinished continuations run on
            trl = topv + hits.to(torch.float32) * -1.0e9
            nxt = torch.topk(trl, k=nb)[1]
            running_seq, running_scores, running_bi = _gather_beams(topk_seq, nxt), _gather_beams(trl, nxt), _gather_beams(topk_bi, nxt)
            # f. finished hypotheses
            just = hits & top_nb[None, :]
            fin = topv / ((cur_len + 1 - W) ** lp)
            fin = fin + (finished.all(-1, keepdim=True) & (es is True)).to(torch.float32) * -1.0e9
            fin = fin + (~improvable).to(torch.float32) * -1.0e9
            fin = fin + (~just) * -1.0e9
            keep = torch.topk(torch.cat((beam_scores, fin), 1), k=nb)[1]
            sequences = _gather_beams(torch.cat((sequences, topk_seq), 1), keep)
            beam_scores = _gather_beams(torch.cat((beam_scores, fin), 1), keep)
            beam_indices = _gather_beams(torch.cat((beam_indices, topk_bi), 1), keep)
            finished = _gather_beams(torch.cat((finished, just), 1), keep)
            # g. early-stop heuristic and the loop condition
            parent = running_bi[..., cur_len - W].reshape(R)
            cur_len += 1
            best_len = (max_length if es == "never" and lp > 0.0 else cur_len) - W
            worst = torch.where(finished, beam_scores.min(1, keepdim=True)[0], -1.0e9)
            improvable = improvable & (running_scores[:, :1] / (best_len ** lp) > worst).any(-1, keepdim=True)
            go = improvable.any() & ~(finished.all() & (es is True)) & ~hits.all()
            if not bool(go):
                break
            # the cache follows its beams: generated rows [prompt_len, seq_len) of every slot from its parent slot
            if cur_len - 1 > W:
                ops.kv_gather(kv.k, kv.v, kv.k, kv.v, parent.contiguous(), row0, cache.seq_len, cur_len - 1 - W, ws=kv_ws)
            o = self.forward(input_ids=running_seq[:, :, cur_len - 1].reshape(R, 1), past_key_values=cache, use_cache=True)
            nxt_logits = o.logits[:, -1]

        sequences = sequences[:, :nrs].reshape(B * nrs, -1)
        beam_scores = beam_scores[:, :nrs].reshape(B * nrs)
        beam_indices = beam_indices[:, :nrs].reshape(B * nrs, -1)
        n_gen = int((beam_indices + 1).bool().sum(1).max())
        sequences, beam_indices = sequences[:, :W + n_gen], beam_indices[:, :n_gen]
        if not cfg.get("return_dict_in_generate"):
            return sequences
        return SimpleNamespace(sequences=sequences, sequences_scores=beam_scores if out_scores else None,
                               scores=tuple(scores) if out_scores else None, logits=tuple(raw) if out_logits else None,
                               beam_indices=beam_indices, attentions=None, hidden_states=None, past_key_values=None)

    # ---- greedy generation (GenerationMixin.generate, do_sample=False)
    @torch.no_grad()
    def _generate_greedy(self, input_ids, input_features=None, attention_mask=None, feature_attention_mask=None, max_new_tokens: int = 20,
                         eos_token_id=None, pad_token_id=None):
        """Greedy decoding: returns [B, L + n_new] = the prompt ids followed by the generated ones; a sequence that has emitted
        `eos_token_id` is continued with `pad_token_id` (HF semantics), generation stops when every sequence has finished."""
        dev = self.device
        eos, pad = self._eos_pad(eos_token_id, pad_token_id)
        input_ids = input_ids.to(dev)
        hid, cache, mask, _, _, _ = self._prefill(input_ids, input_features, attention_mask, feature_attention_mask, None, None, max_new_tokens)
        B = input_ids.shape[0]
        # the last VALID token of each prompt, wherever the padding sits (the reference's generate() reads column -1, i.e. needs
        # left padding; the compact layout does not care)
        nxt_logits = self._head(hid[torch.arange(B, device=dev), cache.seq_len.long() - 1]).to(self.dtype)
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        new = []
        for step in range(max_new_tokens):
            tok = nxt_logits.argmax(-1)
            tok = torch.where(unfinished, tok, torch.full_like(tok, pad))
            new.append(tok)
            for e in eos:
                unfinished = unfinished & (tok != e)
            if not bool(unfinished.any()) or step == max_new_tokens - 1:
                break
            o = self.forward(input_ids=tok[:, None], past_key_values=cache, use_cache=True)
            nxt_logits, cache = o.logits[:, -1], o.past_key_values
        return torch.cat([input_ids, torch.stack(new, dim=1)], dim=1)
