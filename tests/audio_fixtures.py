"""How the mel fixtures (tests/golden/melspec.npz, melspec_meta.json) are built and restated: shared by
tools/make_golden_melspec.py, which writes them with the reference's own mel_spectrogram, and the audio tests."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SR, N_FFT, HOP, PAD = 22050, 1024, 256, 384
LENGTHS = (385, 1024, 2660, 16384, 22050)          # samples; frames = L // 256 = 1, 4, 10, 64, 86
SEEDS = {385: 31, 1024: 32, 2660: 33, 16384: 34, 22050: 35}
ZEROS = 3000                                       # a stretch of exact zeros from L // 2 on: hits the 1e-5 clamp


def make_wave(L: int, seed: int) -> np.ndarray:
    """voiced-like: 29 harmonics at 1/h of a 140 +- 40 Hz contour, peak 0.3, white noise at 0.01 rms, digital silence
    in [L // 2, L // 2 + 3000)."""
    rng = np.random.RandomState(seed)
    t = np.arange(L, dtype=np.float64) / SR
    f0 = 140.0 + 40.0 * np.sin(2.0 * np.pi * 1.5 * t + rng.uniform(0.0, 2.0 * np.pi))
    phase = 2.0 * np.pi * np.cumsum(f0) / SR
    x = sum(np.sin(h * phase) / h for h in range(1, 30))
    x = 0.3 * x / np.abs(x).max() + 0.01 * rng.standard_normal(L)
    x[L // 2:L // 2 + ZEROS] = 0.0
    return x.astype(np.float32)


def reflect_pad(x: np.ndarray) -> np.ndarray:
    L = x.shape[0]
    s = np.arange(-PAD, L + PAD)
    s = np.where(s < 0, -s, np.where(s >= L, 2 * (L - 1) - s, s))
    return x[s]


def frames_of(x: np.ndarray) -> np.ndarray:
    """[T, 1024] padded frames of x, T = L // 256."""
    y = reflect_pad(x)
    T = x.shape[0] // HOP
    return np.stack([y[HOP * t:HOP * t + N_FFT] for t in range(T)])


def mel_fp64(x: np.ndarray, basis: np.ndarray) -> np.ndarray:
    """the five steps in fp64 numpy: reflect pad, Hann frames, real DFT magnitude (+1e-9 under the root), filterbank,
    log(clamp(., 1e-5)) -> [80, T]."""
    n = np.arange(N_FFT)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)
    spec = np.fft.rfft(frames_of(x.astype(np.float64)) * hann, axis=1)
    mag = np.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    return np.log(np.maximum(basis.astype(np.float64) @ mag.T, 1e-5))


def load():
    """-> ({L: wav}, {L: reference mel [80, T]}, basis [80, 513], meta)"""
    z = np.load(os.path.join(GOLD, "melspec.npz"))
    meta = json.load(open(os.path.join(GOLD, "melspec_meta.json")))
    return ({L: z[f"wav_{L}"] for L in LENGTHS}, {L: z[f"mel_{L}"] for L in LENGTHS}, z["basis"], meta)
