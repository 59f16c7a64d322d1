"""ContinuousAudioIO on MI355X: the audio-input plugin of UALM (log-mel + AF-Whisper encoder) over HIP.

Mirrors `ContinuousAudioIO` (UALM/models/ualm/multimodal_io/audio.py:873-1262): same constructor arguments,
`preprocess` / `encode_batch` / `find_length` / `copy_for_worker` / `feature_dim`, same attributes
(`model`, `processor`, `d_model`, `sample_rate`, `hop_length`, `n_samples`).  The key-padding mask of
encode_batch is handed to the kernels as the per-clip length vector the reference derives it from
(audio.py:1135-1142); the [B,1,1500,1500] tensor is never built.
"""
from typing import List, Tuple

import numpy as np
import os
import torch

from .. import _lib as L
from . import resample
from .abs_io import AbsIO
from .feature_extraction import WhisperFeatureExtractorHIP
from .modeling_whisper import AFWhisperEncoder


class ContinuousAudioIO(AbsIO):
    def __init__(self, encoder_choice: str = "AFWhisper", encoder_hf_model_tag: str = "Qwen/Qwen2.5-Omni-7B",
                 encoder_local_path: str = None, attn_implementation: str = None, dtype: str = "bfloat16",
                 device: str = "cuda", _skip_loading: bool = False, encoder: AFWhisperEncoder = None):
        super().__init__(modality="audio", is_discrete=False)
        self.device = device
        self.encoder_choice = encoder_choice
        self.encoder_hf_model_tag = encoder_hf_model_tag
        self.encoder_local_path = encoder_local_path
        self.attn_implementation = attn_implementation   # accepted for signature parity; attention is always the fused kernel
        self.dtype_str = dtype
        self.dtype = getattr(torch, dtype)
        if _skip_loading:
            self.model = None
            self.processor = None
        else:
            self._init_encoder(encoder)

    def _init_encoder(self, encoder=None):
        if self.encoder_choice != "AFWhisper":
            # audio.py:929-959: the "huggingface" choice fetches Qwen/Qwen2.5-Omni-7B from the network
            raise NotImplementedError(f"Encoder choice {self.encoder_choice} not implemented (AF-Whisper by local path only)")
        if encoder is None:
            if self.encoder_local_path is None:
                raise ValueError("encoder_local_path must be provided for AFWhisper encoder choice")
            encoder = AFWhisperEncoder.from_pretrained(self.encoder_local_path, torch_dtype=self.dtype)
        self.model = encoder.to(device=self.device, dtype=self.dtype)
        self.model.eval()
        self.processor = WhisperFeatureExtractorHIP(feature_size=self.model.config.num_mel_bins, sampling_rate=16000,
                                                    hop_length=160, n_fft=400, padding_value=0.0)
        self.d_model = self.model.config.d_model
        self.sample_rate = self.processor.sampling_rate
        self.hop_length = self.processor.hop_length
        self.n_samples = self.model.config.max_source_positions * 2 * self.hop_length

    # ------------------------------------------------------------------ CPU-facing API (numpy in / numpy out)
    def _after_length(self, n_samples: int) -> int:
        before = n_samples // self.hop_length
        after = (before - 1) // 2 + 1
        return int((after - 2) // 2 + 1)

    def preprocess(self, data: Tuple[np.ndarray, int]):
        """audio.py:1013-1101: (wav, sr) -> (zeros[after,1] int32, (after, mel[3000,128] f32), zeros[after,1])."""
        wav, fs = data
        import torch.utils.data as _tud
        if _tud.get_worker_info() is not None:
            # the reference's worker copy computes the mel on the CPU; here the log-mel IS a HIP kernel, and a forked DataLoader worker
            # cannot re-initialise the HIP runtime (a spawned one would open one GPU context per worker)
            raise RuntimeError("ContinuousAudioIO.preprocess runs the log-mel kernel on the GPU: call it in the main process "
                               "(DataLoader num_workers=0), or feed raw waveforms to encode_wav_batch")
        if fs != self.sample_rate:
            return self._preprocess_resampled(wav, int(fs))
        if len(wav.shape) > 1:
            wav = wav[0]
        if wav.shape[0] > self.n_samples:
            print(f"Warning: Input audio is too long to process, will truncate to {self.n_samples} samples")
            wav = wav[: self.n_samples]
        if not isinstance(wav, np.ndarray):
            wav = np.array(wav)
        original_samples = wav.shape[0]
        feat = self.processor(wav, sampling_rate=self.sample_rate, return_tensors="np")["input_features"][0].T
        after_length = self._after_length(original_samples)
        paddings = np.zeros((after_length, 1)).astype(np.int32)
        return paddings, (after_length, np.ascontiguousarray(feat)), paddings

    def _preprocess_resampled(self, wav, fs: int):
        """preprocess for a clip at fs > 16 kHz, in the reference's order (audio.py:1031-1044): resample (GPU), first channel, truncate
        to n_samples, then the log-mel of the device buffer.  Only the first channel is uploaded and resampled -- the reference resamples
        every channel and keeps wav[0], the same samples.  Only the first n_samples outputs are computed: each output depends on the
        input alone, so they equal the head of the fully resampled clip."""
        resample.check_front_end_rate(fs, self.sample_rate)     # below 16 kHz, or an unsupported pair: raises here
        wav = np.asarray(wav)
        if wav.ndim > 1:
            wav = wav[0]
        n_res = resample.out_length(wav.shape[0], fs, self.sample_rate)
        if n_res > self.n_samples:
            print(f"Warning: Input audio is too long to process, will truncate to {self.n_samples} samples")
        n = min(n_res, self.n_samples)
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        if dev is None:
            L.lib()  # raises: no CPU fallback
        x = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(dev)
        y, _ = resample.resample_device(x[None], fs, self.sample_rate, n_out=n)
        feat = self.processor.extract_device(y, layout="bct")[0].cpu().numpy().T
        after_length = self._after_length(n)
        paddings = np.zeros((after_length, 1)).astype(np.int32)
        return paddings, (after_length, np.ascontiguousarray(feat)), paddings

    def find_length(self, data: Tuple[np.ndarray, int]) -> int:
        """audio.py:1189-1214."""
        wav, sr = data
        num_samples = int(wav.shape[-1] * self.sample_rate / sr) if sr != self.sample_rate else wav.shape[-1]
        return self._after_length(num_samples)

    # ------------------------------------------------------------------ GPU API
    @torch.no_grad()
    def encode_batch(self, batch_data: torch.Tensor, length: torch.Tensor) -> List[torch.Tensor]:
        """audio.py:1103-1187: mel [B,3000,128] + length[B] -> list of [out_len_i, d_model] tensors.

        `length` follows the caller's convention (SURVEY headline fact 5): the pipeline passes 3000 (no key is
        masked, all 750 rows returned); the self-test passes after_length (keys >= feat_len masked, rows trimmed)."""
        if self.model is None:
            raise RuntimeError("worker copy has no encoder (copy_for_worker)")
        input_mel_lengths = length.to(torch.long).cpu() * 4 - 1
        feat_len, out_len = self.model._get_feat_extract_output_lengths(input_mel_lengths)
        Tp = self.model.config.max_source_positions
        feat_len = feat_len.clamp(max=Tp)
        # clips of different lengths (self-test convention): the encoder runs on the valid positions only, packed -- the rows
        # returned below are bit-identical to the padded forward, the ones it would compute from padding are trimmed anyway
        ragged = bool((feat_len < Tp).any()) and os.environ.get("AFHIP_ENCODER_RAGGED", "1") != "0"
        out = self.model.encode_btc(batch_data, feat_len=feat_len, ragged=ragged)
        return [out[i, : int(out_len[i])] for i in range(out.shape[0])]

    @torch.no_grad()
    def encode_wav_batch(self, wav: torch.Tensor, length: torch.Tensor = None, sample_rate: int = 16000,
                         n_valid: torch.Tensor = None) -> List[torch.Tensor]:
        """Fused device path: raw clips [B, n] f32 on the GPU -> encoder outputs, no host hop.
        `length` as in encode_batch (default: pipeline convention, 3000).  16 kHz clips go straight to the log-mel (n <= 480000 is used,
        as before).  Clips at a supported `sample_rate` above 16 kHz are resampled on the GPU first (the first 480000 outputs, the reference's
        truncation), then the log-mel reads the resampled buffer; `n_valid` [B] is then each clip's valid samples at `sample_rate`
        (default: n), and outputs past a clip's own resampled length are zeros, as padding of a 16 kHz batch is."""
        if sample_rate != self.sample_rate:
            resample.check_front_end_rate(sample_rate, self.sample_rate)
            n_in = wav.shape[1] if n_valid is None else None
            n = self.n_samples if n_in is None else min(resample.out_length(n_in, sample_rate, self.sample_rate), self.n_samples)
            wav, _ = resample.resample_device(wav, sample_rate, self.sample_rate, lengths=n_valid, n_out=n)
        mel = self.processor.extract_device(wav, layout="btc", dtype=self.dtype)
        if length is None:
            length = torch.full((wav.shape[0],), 3000, dtype=torch.long)
        return self.encode_batch(mel, length)

    def copy_for_worker(self) -> "ContinuousAudioIO":
        """audio.py:1216-1254: model-less copy that keeps processor + metadata."""
        c = self.__class__(encoder_choice=self.encoder_choice, encoder_hf_model_tag=self.encoder_hf_model_tag,
                           encoder_local_path=self.encoder_local_path, attn_implementation=self.attn_implementation,
                           dtype=self.dtype_str, device="cpu", _skip_loading=True)
        c.processor = self.processor
        c.d_model, c.sample_rate, c.hop_length, c.n_samples = self.d_model, self.sample_rate, self.hop_length, self.n_samples
        return c

    def feature_dim(self) -> int:
        return self.d_model


# ---------------------------------------------------------------------------------------------------------------------
# Audio-OUTPUT token bookkeeping.  The reference's DiscreteAudioIO (audio.py:68-870) wraps codec / SSL models that
# must be fetched from the network; what the decode loop needs from it is the vocabulary / stream-interval contract and the
# delay (de)interleave of the 8 codebook streams.  The waveform itself (X-codec decode, audio.py:544-596) is outside the path.
def delay_interleave(codes: torch.Tensor, pad_ids) -> torch.Tensor:
    """audio.py:758-782: stream n is delayed by n frames; [B, T, N] -> [B, T + N - 1, N], vacated slots hold the stream's pad id
    (the first id of its interval)."""
    B, T, N = codes.shape
    out = torch.as_tensor(list(pad_ids), dtype=torch.long, device=codes.device).tile(B, T + N - 1, 1)
    for n in range(N):
        out[:, n:n + T, n] = codes[:, :, n]
    return out


def delay_deinterleave(codes: torch.Tensor) -> torch.Tensor:
    """audio.py:785-808: inverse of delay_interleave; [B, T, N] -> [B, T - N + 1, N]."""
    _, T, N = codes.shape
    T0 = T - N + 1
    return torch.stack([codes[:, n:n + T0, n] for n in range(N)], dim=-1)


class DiscreteAudioTokenIO(AbsIO):
    """The part of DiscreteAudioIO the LLM side depends on: `num_stream` codebook streams of `codebook_size` entries (+1 pad id
    each, audio.py:301-414), their vocabulary and stream intervals, and `decode_batch` up to the codec call: unified-vocabulary
    ids [B, T, S] -> de-interleaved codec codes [B, T - S + 1, S] (audio.py:494-541).  Without a codec model `decode_batch` returns the
    codes; with one attached (`attach_codec`: the reference's `codec_choice == "Xcodec"` object, `transformers.XcodecModel`, which the
    reference fetches by tag, audio.py:203-218) it finishes the reference's method -- `_codec_decode_batch`, audio.py:573-588 -- and returns
    (audio [B, 1, samples], sample lengths, sample_rate).  The codec network itself is the caller's HF module and runs where it lives; it
    is not part of the HIP path."""

    def __init__(self, n_stream: int = 8, codebook_size: int = 1024, delay_interleave: bool = True):
        super().__init__(modality="audio", is_discrete=True)
        self.n_stream, self.codebook_size, self.delay = n_stream, codebook_size, delay_interleave
        self._stream_intervals = None
        object.__setattr__(self, "codec_model", None)
        self.sample_rate, self.frame_shift, self.codec_bandwidth = None, None, None

    def attach_codec(self, codec_model):
        """audio.py:203-233: the X-codec object, the two facts the IO takes from its config, and the target bandwidth closest to
        `n_stream` quantizers (log2(codebook) bits x frames per second each)."""
        import math
        # kept OUT of the module tree on purpose: the drop-in's state-dict keys stay those of the checkpoint (strict=True loads), and the
        # codec lives on whatever device its owner put it
        object.__setattr__(self, "codec_model", codec_model)
        self.sample_rate = codec_model.config.sample_rate
        self.frame_shift = codec_model.config.hop_length
        per_q = math.log2(codec_model.config.codebook_size) * (self.sample_rate // self.frame_shift) / 1000      # kbps
        want = per_q * self.n_stream
        self.codec_bandwidth = min(codec_model.config.target_bandwidths, key=lambda x: abs(x - want))
        return self

    def find_length(self, data):
        """audio.py:656-672: frames a clip (wav [ch, samples], sample rate) becomes, delay interleave included."""
        if self.codec_model is None:
            raise RuntimeError("DiscreteAudioTokenIO.find_length needs a codec (attach_codec)")
        wav, sr = data
        num_samples = wav.shape[-1] * self.sample_rate / sr
        return int(num_samples // self.frame_shift) + (self.n_stream - 1 if self.delay else 0)

    def encode_batch(self, data: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """audio.py:417-491 for the codec-only configuration (no SSL streams: their tokeniser is not importable here):
        wav [B, samples, channels] + sample lengths [B] -> ids [B, frames (+ n_stream - 1), n_stream] in the IO's own vocabulary
        (stream offset + 1, slot 0 of a stream = pad), delay-interleaved.  The codec is the attached HF module (audio.py:641-654)."""
        if self.codec_model is None:
            raise RuntimeError("DiscreteAudioTokenIO.encode_batch needs a codec (attach_codec): on-the-fly tokenisation has no other source")
        if data.dim() != 3:
            raise ValueError(f"Expected 3D tensor [batch, samples, num_channel], got {data.dim()}D")
        data = data.transpose(1, 2)
        frame_lengths = lengths // self.frame_shift
        lengths = frame_lengths * self.frame_shift
        data = data[:, :, : int(lengths.max())]
        codec_codes = self.codec_model.encode(data[:, :1, : int(lengths.max())], bandwidth=self.codec_bandwidth, return_dict=False)
        codec_codes = codec_codes.permute(0, 2, 1)[:, :, : self.n_stream]                       # [B, T, S]
        max_frames = int(frame_lengths.max())
        cur = codec_codes.size(1)
        if cur > max_frames:
            codec_codes = codec_codes[:, :max_frames]
        elif cur < max_frames:
            codec_codes = torch.nn.functional.pad(codec_codes, (0, 0, 0, max_frames - cur), mode="replicate")
        codes = codec_codes.to(torch.long).clone()
        pads = []
        for s, (start, _) in enumerate(self.get_stream_interval()):
            codes[..., s] += start + 1
            pads.append(start)
        if self.delay:
            codes = delay_interleave(codes, pads)
        return codes

    def num_stream(self):
        return self.n_stream

    def get_vocabulary(self):
        return [f"<audio_{i}>" for i in range(self.n_stream * (self.codebook_size + 1))]

    def get_stream_interval(self):
        w = self.codebook_size + 1
        return [(s * w, (s + 1) * w) for s in range(self.n_stream)]

    def set_vocab_offset(self, intervals):
        """absolute intervals of the unified vocabulary (vocab_intervals["discrete_audio"], ualm_job.py:96-104)"""
        self._stream_intervals = [tuple(iv) for iv in intervals]

    def copy_for_worker(self):
        return self

    def decode_batch(self, codes: torch.Tensor, lengths: torch.Tensor):
        if codes.dim() != 3:
            raise ValueError(f"Expected 3D token tensor [batch, time, n_streams], got {codes.dim()}D")
        if self.delay:
            codes = delay_deinterleave(codes)
            lengths = lengths - self.num_stream() + 1
        codes = codes.clone()
        for s, (start, _) in enumerate(self.get_stream_interval()):
            codes[..., s] -= start + 1                  # ids relative to the IO's own vocabulary; slot 0 of a stream is its pad
        if self.codec_model is None:
            return codes, lengths
        # audio.py:573-588 (_codec_decode_batch, Xcodec branch): [B, T, S] -> [B, S, T], pad ids (-1) decode as entry 0
        c = codes.permute(0, 2, 1)
        c = torch.where(c < 0, torch.zeros_like(c), c)
        audio = self.codec_model.decode(c).audio_values
        if audio.dim() == 2:
            audio = audio.unsqueeze(1)
        return audio, lengths * self.frame_shift, self.sample_rate
