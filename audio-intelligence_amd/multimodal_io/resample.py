"""Sample-rate conversion on the GPU in front of the log-mel (csrc/resample.hip): the device form of the
`librosa.resample(wav, orig_sr=fs, target_sr=16000)` call in ContinuousAudioIO.preprocess (audio.py:1031-1034).

Filter (include/afhip.h, afhip_resample): Kaiser-windowed sinc, cutoff 0.955 f_min/2, 110 dB, linear phase -- the class of soxr's HQ
recipe, not soxr's filter.  Sample convention: librosa's, output length ceil(n fs_out / fs_in).  The [L][T_pad] coefficient table of a
rate pair is built by the library on the host in double and uploaded once per (device, pair).
"""
import ctypes as C
import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib as L

_tables = {}          # (device index, fs_in, fs_out) -> f32 tensor [L * T_pad] on that device


def plan(fs_in: int, fs_out: int) -> Tuple[int, int, int, int]:
    """(L, M, K, T_pad) of a rate pair; raises AfhipError (with the library's message) for an unsupported pair."""
    lib = L.load_library()
    out = [C.c_int() for _ in range(4)]
    L.check(lib.afhip_resample_plan(int(fs_in), int(fs_out), *[C.byref(v) for v in out]))
    return tuple(v.value for v in out)


def check_front_end_rate(fs: int, target: int = 16000):
    """The audio front end (ContinuousAudioIO.preprocess / encode_wav_batch, long_audio_inference) converts DOWN to 16 kHz: input below
    it raises ValueError, as all non-16-kHz input did before, and input above it must be a pair the resampler supports (AfhipError
    naming the pair otherwise).  Up-sampling is available from resample_device for a caller that wants it."""
    if int(fs) < int(target):
        raise ValueError(f"sampling rate {fs} < {target}: the audio front end converts down to {target} Hz only; up-sample first "
                         f"(multimodal_io.resample.resample_device(wav, {fs}, {target}) does it on the GPU)")
    plan(fs, target)


def out_length(n_in: int, fs_in: int, fs_out: int) -> int:
    """Resampled length of an n_in-sample clip: ceil(n_in fs_out / fs_in) (librosa's fix_length size)."""
    return -(-int(n_in) * int(fs_out) // int(fs_in))


def span_period(fs_in: int, fs_out: int) -> Tuple[int, int]:
    """(inputs, outputs) of one period of the kernel's sum order: an input span that starts at a multiple of `inputs` samples,
    resampled from m0 - (its start / inputs) * outputs, gives outputs bit-identical to those of the whole clip (afhip.h)."""
    Lr, Mr, _, _ = plan(fs_in, fs_out)
    P = 16 // math.gcd(Lr, 16)
    return P * Mr, P * Lr


def input_span(m_lo: int, m_hi: int, n_in: int, fs_in: int, fs_out: int) -> Tuple[int, int, int]:
    """Input samples [s0, s1) that outputs [m_lo, m_hi) of an n_in-sample clip read (+-K taps), with s0 on a span_period boundary,
    and the m0 to pass for them when the span is resampled on its own: returns (s0, s1, m0)."""
    Lr, Mr, K, _ = plan(fs_in, fs_out)
    per_in, per_out = span_period(fs_in, fs_out)
    first = (m_lo * Mr) // Lr - K
    last = ((m_hi - 1) * Mr) // Lr + K
    j = max(first, 0) // per_in
    s0 = j * per_in
    s1 = min(max(last + 1, s0), n_in)
    return s0, s1, m_lo - j * per_out


def _device_tables(device: torch.device, fs_in: int, fs_out: int) -> torch.Tensor:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, int(fs_in), int(fs_out))
    if key not in _tables:
        lib = L.lib()
        Lr, _, _, T_pad = plan(fs_in, fs_out)
        host = np.zeros(Lr * T_pad, dtype=np.float32)
        L.check(lib.afhip_resample_tables_host(int(fs_in), int(fs_out), host.ctypes.data_as(C.c_void_p)))
        _tables[key] = torch.from_numpy(host).to(device)
    return _tables[key]


def resample_device(wav: torch.Tensor, orig_sr: int, target_sr: int = 16000,
                    lengths: Optional[Union[torch.Tensor, Sequence[int]]] = None, m0: int = 0,
                    n_out: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """wav [B, n] (or [n]) f32 on the GPU, `lengths` [B] valid samples per clip (default: n) -> (y [B, n_out] f32, out_lengths [B]).

    y holds outputs [m0, m0 + n_out) of every clip resampled from orig_sr to target_sr; outputs at or past a clip's own resampled length
    ceil(lengths[b] target_sr / orig_sr) are zeros.  `n_out` defaults to the longest clip's resampled length minus m0 (with device-resident
    `lengths` that default costs one device-to-host read).  out_lengths[b] = clamp(ceil(lengths[b] target_sr / orig_sr) - m0, 0, n_out)
    (int64, on wav's device).  orig_sr == target_sr returns wav itself (and its lengths) without a launch."""
    if not wav.is_cuda or wav.dtype != torch.float32 or wav.dim() not in (1, 2):
        raise L.AfhipError("resample_device expects a float32 CUDA/HIP tensor [B, n_samples] or [n_samples]")
    squeeze = wav.dim() == 1
    if squeeze:
        wav = wav[None]
    B, n = wav.shape
    if lengths is None:
        lens = torch.full((B,), n, dtype=torch.int32, device=wav.device)
        n_max = n
    else:
        lens = torch.as_tensor(lengths)
        if lens.shape != (B,):
            raise L.AfhipError(f"resample_device: lengths has shape {tuple(lens.shape)}, expected ({B},)")
        n_max = None if (n_out is not None or int(orig_sr) == int(target_sr)) else int(lens.max())
        lens = lens.to(device=wav.device, dtype=torch.int32)
    if int(orig_sr) == int(target_sr):
        return (wav[0] if squeeze else wav), lens.to(torch.int64)
    lib = L.lib()
    if n_out is None:
        n_out = max(out_length(n_max, orig_sr, target_sr) - int(m0), 1)
    if wav.stride(1) != 1:
        wav = wav.contiguous()
    x_stride = wav.stride(0) if B > 1 else n          # torch reports arbitrary strides for size-1 dims
    y = torch.empty((B, int(n_out)), dtype=torch.float32, device=wav.device)
    L.check(lib.afhip_resample(L.ptr(wav), B, L.ptr(lens), x_stride, L.ptr(y), int(m0), int(n_out), int(n_out), int(orig_sr),
                               int(target_sr), L.ptr(_device_tables(wav.device, orig_sr, target_sr)), L.stream_ptr()))
    out_len = ((lens.to(torch.int64) * int(target_sr) + int(orig_sr) - 1) // int(orig_sr) - int(m0)).clamp(0, int(n_out))
    return (y[0] if squeeze else y), out_len
