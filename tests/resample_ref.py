"""float64 numpy restatement of the resampler's filter and sample convention (include/afhip.h, afhip_resample): the table the
library builds, the polyphase sum and the length rules.  Test support only; imports nothing from the package."""
import math

import numpy as np

STANDARD_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)


def plan(fs_in: int, fs_out: int):
    """(L, M, K, T_pad) of a rate pair."""
    g = math.gcd(fs_in, fs_out)
    L, M = fs_out // g, fs_in // g
    fmin = float(min(fs_in, fs_out))
    delta = 0.09 * fmin / 2.0
    th = (110.0 - 7.95) / (4.57 * 2.0 * math.pi * delta)
    K = int(math.ceil(th * fs_in))
    return L, M, K, (2 * K + 1 + 3) // 4 * 4


def half_width(fs_in: int, fs_out: int) -> float:
    """T_h in seconds."""
    fmin = float(min(fs_in, fs_out))
    return (110.0 - 7.95) / (4.57 * 2.0 * math.pi * 0.09 * fmin / 2.0)


def h(tau, fs_in: int, fs_out: int):
    """The Kaiser-windowed sinc at offsets tau (seconds)."""
    fmin = float(min(fs_in, fs_out))
    fc = 0.955 * fmin / 2.0
    beta = 0.1102 * (110.0 - 8.7)
    th = half_width(fs_in, fs_out)
    tau = np.asarray(tau, dtype=np.float64)
    r = tau / th
    inside = np.abs(r) <= 1.0
    win = np.i0(beta * np.sqrt(np.clip(1.0 - r * r, 0.0, None))) / np.i0(beta)
    return np.where(inside, (2.0 * fc / fs_in) * np.sinc(2.0 * fc * tau) * win, 0.0)


def table(fs_in: int, fs_out: int) -> np.ndarray:
    """[L][T_pad] float64: H[p][k + K] = h((p/L - k) / fs_in), zero padded."""
    L, M, K, T_pad = plan(fs_in, fs_out)
    p = np.arange(L, dtype=np.float64)[:, None]
    k = np.arange(-K, K + 1, dtype=np.float64)[None, :]
    out = np.zeros((L, T_pad))
    out[:, : 2 * K + 1] = h((p / L - k) / fs_in, fs_in, fs_out)
    return out


def n_out(n_in: int, fs_in: int, fs_out: int) -> int:
    """ceil(n_in fs_out / fs_in): librosa's fix_length size."""
    return -(-n_in * fs_out // fs_in)


def resample_f64(x, fs_in: int, fs_out: int, table_=None, m0: int = 0, count=None) -> np.ndarray:
    """Outputs [m0, m0 + count) (default: all n_out) of the polyphase sum in float64, over `table_` (default: the float64 table;
    pass the library's f32 table to isolate the kernel's accumulation error)."""
    x = np.asarray(x, dtype=np.float64)
    L, M, K, T_pad = plan(fs_in, fs_out)
    H = table(fs_in, fs_out) if table_ is None else np.asarray(table_, dtype=np.float64)
    n = x.shape[0]
    if count is None:
        count = n_out(n, fs_in, fs_out) - m0
    m = np.arange(m0, m0 + count, dtype=np.int64)
    q, p = (m * M) // L, (m * M) % L
    xp = np.concatenate([np.zeros(K), x, np.zeros(K + 1)])
    y = np.zeros(count)
    for j in range(2 * K + 1):            # tap j reads x[q - K + j] = xp[q + j]
        idx = q + j
        y += np.where(idx < xp.shape[0], xp[np.minimum(idx, xp.shape[0] - 1)], 0.0) * H[p, j]
    y[m >= n_out(n, fs_in, fs_out)] = 0.0
    return y
