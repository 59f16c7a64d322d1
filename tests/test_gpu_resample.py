"""GPU resampler (csrc/resample.hip) and the paths built on it: the kernel against the float64 restatement of tests/resample_ref.py over
the library's own f32 table (accumulation error only), the signal contract against analytic tones (table-independent), and
ContinuousAudioIO.preprocess / encode_wav_batch / UALMPreprocessor / long_audio_inference at rates other than 16 kHz."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from oracle import fixtures_common as fc
from tests import helpers as H
from tests import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")


def _f32_table(fs_in, fs_out):
    from audio_intelligence_amd import _lib as L
    Lr, _, _, T_pad = R.plan(fs_in, fs_out)
    buf = np.zeros(Lr * T_pad, dtype=np.float32)
    assert L.load_library().afhip_resample_tables_host(fs_in, fs_out, buf.ctypes.data_as(C.c_void_p)) == 0
    return buf.reshape(Lr, T_pad)


def _rs(x, fs_in, fs_out=16000, **kw):
    from audio_intelligence_amd.multimodal_io.resample import resample_device
    return resample_device(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV), fs_in, fs_out, **kw)


@pytest.mark.parametrize("fs_in,fs_out", [(fs, 16000) for fs in R.STANDARD_RATES if fs != 16000] + [(16000, 44100)])
def test_kernel_matches_f64_restatement_over_f32_table(fs_in, fs_out):
    _need_gpu()
    x = fc.make_wav(fs_in % 1000 + 5, fs_in + 12345)
    y, n = _rs(x, fs_in, fs_out)
    ref = R.resample_f64(x, fs_in, fs_out, _f32_table(fs_in, fs_out))
    assert y.shape[0] == R.n_out(len(x), fs_in, fs_out) == int(n)
    err = float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max())
    assert err <= 4e-6 * float(np.abs(x).max()), err


def test_kernel_ragged_batch_strided_rows_and_zero_tail():
    """One launch over clips of 1, 100 (shorter than the filter), 123 457 and 1 323 000 samples at 44.1 kHz in rows wider than the
    longest clip: every clip matches its own restatement, and every position past its own n_out is an exact zero."""
    _need_gpu()
    from audio_intelligence_amd.multimodal_io.resample import resample_device
    fs = 44100
    lens = [1, 100, 123457, 1323000]
    big = np.zeros((4, 1323000 + 37), np.float32)
    clips = [fc.make_wav(70 + i, n) for i, n in enumerate(lens)]
    for i, c in enumerate(clips):
        big[i, : len(c)] = c
        big[i, len(c):] = 7.0                      # garbage past the valid length must not be read
    xt = torch.from_numpy(big).to(DEV)[:, :1323000]
    assert xt.stride(0) == 1323037
    y, out_len = resample_device(xt, fs, 16000, lengths=torch.tensor(lens, dtype=torch.int32))
    y = y.cpu().numpy()
    assert y.shape == (4, 480000)
    assert out_len.cpu().tolist() == [R.n_out(n, fs, 16000) for n in lens]
    tab = _f32_table(fs, 16000)
    for i, c in enumerate(clips):
        no = R.n_out(len(c), fs, 16000)
        ref = R.resample_f64(c, fs, 16000, tab)
        err = float(np.abs(y[i, :no].astype(np.float64) - ref).max())
        assert err <= 4e-6 * float(np.abs(c).max()), (i, err)
        assert np.all(y[i, no:] == 0.0), i


@pytest.mark.parametrize("fs_in,m0,count", [(44100, 12345, 5000), (48000, 143990, 20), (22050, 1, 70000)])
def test_kernel_window_from_m0(fs_in, m0, count):
    _need_gpu()
    x = fc.make_wav(9, 3 * fs_in)
    y, n = _rs(x, fs_in, m0=m0, n_out=count)
    ref = R.resample_f64(x, fs_in, 16000, _f32_table(fs_in, 16000), m0=m0, count=count)
    assert y.shape[0] == count and int(n) == min(max(R.n_out(len(x), fs_in, 16000) - m0, 0), count)
    assert float(np.abs(y.cpu().numpy() - ref).max()) <= 4e-6 * float(np.abs(x).max())
    # the window is the same range of the whole clip's outputs, bit for bit (the sum order does not depend on m0)
    full, _ = _rs(x, fs_in)
    hi = min(m0 + count, full.shape[0])
    assert torch.equal(y[: hi - m0], full[m0:hi])


def _interior(n_in, fs_in):
    th = R.half_width(fs_in, 16000)
    m = np.arange(R.n_out(n_in, fs_in, 16000))
    return m, (m / 16000 > th) & (m / 16000 < (n_in - 1) / fs_in - th)


@pytest.mark.parametrize("fs_in", [44100, 48000, 22050])
def test_passband_tone_mix_matches_analytic(fs_in):
    _need_gpu()
    n = fs_in // 2
    t = np.arange(n) / fs_in
    freqs, amps = (440.0, 3000.0, 6900.0), (0.5, 0.3, 0.2)
    x = sum(a * np.sin(2 * np.pi * f * t + 0.3) for f, a in zip(freqs, amps))
    y, _ = _rs(x, fs_in)
    m, inner = _interior(n, fs_in)
    ideal = sum(a * np.sin(2 * np.pi * f * m / 16000 + 0.3) for f, a in zip(freqs, amps))
    err = float(np.abs(y.cpu().numpy()[inner] - ideal[inner]).max())
    assert inner.sum() > n // 4 and err <= 3e-5 * sum(amps), err


@pytest.mark.parametrize("fs_in", [44100, 48000, 22050, 96000])
def test_stopband_tones_removed(fs_in):
    _need_gpu()
    n = fs_in // 2
    t = np.arange(n) / fs_in
    m, inner = _interior(n, fs_in)
    for f in (8100.0, 10000.0, 15000.0, 20000.0):
        if f >= fs_in / 2:
            continue
        y, _ = _rs(np.sin(2 * np.pi * f * t), fs_in)
        leak = float(np.abs(y.cpu().numpy()[inner]).max())
        assert leak <= 1e-5, (f, leak)


def _io():
    from audio_intelligence_amd.multimodal_io.audio import ContinuousAudioIO
    from audio_intelligence_amd.multimodal_io.modeling_whisper import AFWhisperEncoder, AFWhisperEncoderConfig
    cfg, sd = H.tiny_enc()
    enc = AFWhisperEncoder(AFWhisperEncoderConfig.from_dict(cfg))
    enc.load_state_dict(sd, strict=True)
    return ContinuousAudioIO(encoder_choice="AFWhisper", dtype="float32", device=DEV, encoder=enc.to(DEV))


def _after(io, n):
    return io._after_length(min(n, 480000))


@pytest.mark.parametrize("fs,n,channels", [(44100, 44100 * 7 + 11, 1), (48000, 48000 * 5 + 3, 2), (44100, 44100 * 40, 1)])
def test_preprocess_resamples_on_the_gpu(fs, n, channels, capsys):
    """preprocess((wav, fs)): the mel of the resampled (then truncated) first channel, <= 1e-4 from the oracle log-mel of the float64
    restatement; after_length from the resampled, truncated length; the 40-s clip is truncated after resampling."""
    _need_gpu()
    io = _io()
    wav = np.stack([fc.make_wav(300 + c, n) for c in range(channels)]) if channels > 1 else fc.make_wav(300, n)
    seq, (after, feat), mask = io.preprocess((wav, fs))
    n16 = R.n_out(n, fs, 16000)
    assert after == _after(io, n16) == seq.shape[0] == mask.shape[0]
    assert ("truncate" in capsys.readouterr().out) == (n16 > 480000)
    first = wav[0] if channels > 1 else wav
    ref_wav = R.resample_f64(first, fs, 16000, count=min(n16, 480000)).astype(np.float32)
    ref = oracle.logmel.log_mel(ref_wav).T
    assert feat.shape == (3000, 128) and feat.dtype == np.float32
    err = float(np.abs(feat - ref).max())
    assert err <= 1e-4, err
    assert io.find_length((wav, fs)) == io._after_length(int(n * 16000 / fs))      # the reference's floor rule stays


def test_encode_wav_batch_resamples_in_front_of_the_log_mel():
    _need_gpu()
    from audio_intelligence_amd.multimodal_io.resample import resample_device
    io = _io()
    n = 48000 * 9 + 5
    wav = torch.from_numpy(np.stack([fc.make_wav(500, n), fc.make_wav(501, n)])).to(DEV)
    fused = io.encode_wav_batch(wav, sample_rate=48000)
    y, _ = resample_device(wav, 48000)
    pre = io.encode_wav_batch(y)
    for a, b in zip(fused, pre):
        assert torch.equal(a, b)
    # ... and the host path: preprocess -> encode_batch
    _, (after, feat), _ = io.preprocess((wav[0].cpu().numpy(), 48000))
    via = io.encode_batch(torch.from_numpy(feat)[None].to(DEV), torch.tensor([3000]))[0]
    assert float((via - fused[0]).abs().max()) <= 2e-4
    # per-clip valid lengths at the input rate
    short = io.encode_wav_batch(wav, sample_rate=48000, n_valid=torch.tensor([n, 48000 * 3], device=DEV))
    y2, _ = resample_device(wav, 48000, lengths=[n, 48000 * 3], n_out=480000)
    assert torch.equal(short[1], io.encode_wav_batch(y2)[1])


def _greedy(model, pre, wav, fs, prompt):
    data = {"audio": (wav[None], fs), "text": [["user", "text", prompt]]}
    b = pre.collate_fn([(("audio_to_caption", "x", "y"), data)])
    kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in b.items() if k not in ("keys", "loss_masks")}
    cfg = {"text": {"temperature": 0.0, "topk": 20, "cfg": 1, "max_step": 8}, "num_hypo": 1}
    hyps, _ = model.inference_segment(cfg, cache=None, enforce_modality="text", **kw)
    return hyps[0][0][:, 0].cpu().tolist()


def test_ualm_preprocessor_takes_44k_audio():
    _need_gpu()
    model, pre = H.build_tiny_ualm(torch.float32, DEV)
    lcfg, _, _, _ = H.tiny_llm()
    prompt = fc.make_prompt(lcfg["text_vocab"])
    wav = fc.make_wav(1234, 44100 * 6 + 17)
    got = _greedy(model, pre, wav, 44100, prompt)
    ref = _greedy(model, pre, R.resample_f64(wav, 44100, 16000).astype(np.float32), 16000, prompt)
    assert got == ref


def test_long_audio_at_44k():
    """A 70-s 44.1 kHz clip: windows resampled from each rank's own input span (the block two ranks would each own) equal the windows
    of the fully resampled clip bit for bit; its greedy ids equal those of the clip pre-resampled in float64 and fed at 16 kHz."""
    _need_gpu()
    from audio_intelligence_amd import long_audio as LA
    from audio_intelligence_amd.multimodal_io.resample import resample_device
    fs = 44100
    clip = fc.make_wav(777, 70 * fs + 123)
    n16 = R.n_out(len(clip), fs, 16000)
    spans = [(0, a, b) for a, b in LA.split_windows(n16)]
    assert len(spans) == 3
    full, _ = resample_device(torch.from_numpy(clip).to(DEV), fs)
    for rank in range(2):
        lo, hi = LA.shard_range(len(spans), rank, 2)
        wins = LA._resampled_windows([clip], spans[lo:hi], fs, torch.device(DEV))
        for i, (_, a, b) in enumerate(spans[lo:hi]):
            assert torch.equal(wins[i, : b - a], full[a:b]), (rank, i)
            assert torch.all(wins[i, b - a:] == 0)
    model, _ = H.build_tiny_ualm(torch.float32, DEV)
    lcfg, _, _, _ = H.tiny_llm()
    io = model.multimodal_io_dict["continuous_audio"]
    prompts = [fc.make_prompt(lcfg["text_vocab"])]
    cfg = {"text": {"temperature": 0.0, "topk": 20, "cfg": 1, "max_step": 12}, "num_hypo": 1}
    got = LA.long_audio_inference(model, io, [clip], prompts, cfg, enforce_modality="text", sample_rate=fs)
    ref = LA.long_audio_inference(model, io, [R.resample_f64(clip, fs, 16000).astype(np.float32)], prompts, cfg, enforce_modality="text")
    assert got[0][0][:, 0].cpu().tolist() == ref[0][0][:, 0].cpu().tolist()
