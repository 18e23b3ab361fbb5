"""Waveform -> the Flow's log-mel features on the GPU: the drop-in for the reference's ``matcha/utils/audio.py``.

``mel_spectrogram`` keeps the reference's signature and layout ([B, 80, T]); ``MelExtractor`` is what the other callers
use (ragged batches, channel-last output, padding value).  Both run ``cvft_melspec`` (csrc/melspec.hip): one launch from
samples to log-mel.  Only the CosyVoice-300M setting is built -- 22 050 Hz, n_fft = window = 1024, hop 256, 80 Slaney
bands over 0 .. 8000 Hz, ``center=False`` -- and every other setting raises ``NotImplementedError`` naming it; audio at
another rate is resampled first, by the caller: ``Resampler`` / ``resample`` run ``cvft_resample`` (csrc/resample.hip), the
published formula of ``torchaudio.transforms.Resample`` with its defaults (``sinc_kernel``).
``whisper_log_mel`` and ``kaldi_fbank`` are the two 16 kHz front-ends of the reference's speech tokenizer and speaker
encoder (``cvft_feat16k``, csrc/feat16k.hip).

``mel_filterbank`` restates the documented formula of ``librosa.filters.mel`` with its defaults (Slaney scale, Slaney
area normalisation) in fp64, rounded once to fp32; it is not a copy of librosa's output.
"""
from __future__ import annotations

import math
import wave
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

SAMPLE_RATE, N_FFT, HOP, WIN, N_MELS, FMIN, FMAX = 22050, 1024, 256, 1024, 80, 0, 8000
REFLECT = (N_FFT - HOP) // 2                 # samples of reflect padding per side
MIN_SAMPLES = REFLECT + 1
LOG_CLAMP = math.log(1e-5)                   # the log-mel of digital silence

_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = 15.0                           # 1000 Hz / (200/3 Hz per mel)
_LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f):
    """Slaney scale: linear below 1 kHz (200/3 Hz per mel), logarithmic above (27 mel per factor 6.4)."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, 1e-300) / _MIN_LOG_HZ) / _LOGSTEP, f * 3.0 / 200.0)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL)), m * 200.0 / 3.0)


def mel_frequencies(n: int, fmin: float, fmax: float) -> np.ndarray:
    """n frequencies (Hz) equally spaced on the mel scale from fmin to fmax."""
    return mel_to_hz(np.linspace(float(hz_to_mel(fmin)), float(hz_to_mel(fmax)), n))


def mel_filterbank(sr: int, n_fft: int, n_mels: int, fmin: float, fmax: Optional[float]) -> np.ndarray:
    """[n_mels, n_fft // 2 + 1] fp32: triangles between neighbouring mel frequencies, row i scaled by
    2 / (f[i+2] - f[i])."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    bins = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    f = mel_frequencies(n_mels + 2, fmin, fmax)
    fdiff = np.diff(f)
    ramps = f[:, None] - bins[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (f[2:] - f[:-2]))[:, None]
    return w.astype(np.float32)


def n_frames(length: int) -> int:
    """frames of a `length`-sample waveform: (length + 2 * 384 - 1024) // 256 + 1 == length // 256."""
    return int(length) // HOP


def pack_dft_table(nchunks: int) -> np.ndarray:
    """the DFT operand of cvft_melspec (include/cvft.h): hann[n] * cos | sin(2 pi (n k mod 1024) / 1024) in fp64, rounded
    once, [chunk][step][cos | sin][lane][e] with k = 16 c + (l & 15), n = 256 (s >> 4) + 64 (l >> 4) + 4 (s & 15) + e."""
    c = np.arange(nchunks).reshape(-1, 1, 1, 1)
    s = np.arange(64).reshape(1, -1, 1, 1)
    lane = np.arange(64).reshape(1, 1, -1, 1)
    e = np.arange(4).reshape(1, 1, 1, -1)
    k = 16 * c + (lane & 15)
    n = 256 * (s >> 4) + 64 * (lane >> 4) + 4 * (s & 15) + e
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / WIN)                  # periodic Hann
    ang = 2.0 * np.pi * ((n * k) % N_FFT) / N_FFT
    live = k <= N_FFT // 2
    tab = np.stack([np.where(live, hann * np.cos(ang), 0.0), np.where(live, hann * np.sin(ang), 0.0)], axis=2)
    return np.ascontiguousarray(tab.astype(np.float32))               # [nchunks, 64, 2, 64, 4]


def pack_basis(basis: np.ndarray, nchunks: int) -> np.ndarray:
    """the filterbank operand of cvft_melspec: [chunk][band tile][lane][i] = basis[16 m + (l & 15)][16 c + 4 (l >> 4) + i]."""
    nb, nbin = basis.shape
    mt = (nb + 15) // 16
    full = np.zeros((16 * mt, 16 * nchunks), dtype=np.float32)
    full[:nb, :min(nbin, 16 * nchunks)] = basis[:, :16 * nchunks]
    c = np.arange(nchunks).reshape(-1, 1, 1, 1)
    m = np.arange(mt).reshape(1, -1, 1, 1)
    lane = np.arange(64).reshape(1, 1, -1, 1)
    i = np.arange(4).reshape(1, 1, 1, -1)
    return np.ascontiguousarray(full[16 * m + (lane & 15), 16 * c + 4 * (lane >> 4) + i])


def live_bins(basis: np.ndarray) -> int:
    """bins that carry filterbank weight: the last non-zero column + 1 (372 of 513 with the top band at 8 kHz)."""
    return int(np.nonzero(basis.any(axis=0))[0][-1]) + 1


def check_rate(rate: int) -> None:
    if int(rate) != SAMPLE_RATE:
        raise NotImplementedError(f"sampling rate {rate} Hz: the mel front-end is built for {SAMPLE_RATE} Hz only (resample first: "
                                  f"audio.resample)")


def load_wav(path: str) -> Tuple[torch.Tensor, int]:
    """integer PCM file -> (float32 samples [L] in [-1, 1), channels averaged; the file's rate).  16-bit samples are
    scaled by 1 / 32768, 8-bit unsigned ones by (v - 128) / 128, 24- and 32-bit ones by 2^-23 and 2^-31."""
    with wave.open(path, 'rb') as f:
        sw = f.getsampwidth()
        if sw not in (1, 2, 3, 4):
            raise NotImplementedError(f"{path}: {8 * sw}-bit samples (8-, 16-, 24- and 32-bit integer PCM is read)")
        rate, ch = f.getframerate(), f.getnchannels()
        raw = f.readframes(f.getnframes())
    if sw == 2:
        x = np.frombuffer(raw, dtype='<i2').astype(np.float32) / 32768.0
    elif sw == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif sw == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float32) / 8388608.0           # |v| < 2^24: exact in fp32
    else:
        x = (np.frombuffer(raw, dtype='<i4').astype(np.float64) / 2147483648.0).astype(np.float32)
    if ch > 1:
        x = x.reshape(-1, ch).mean(axis=1, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(x)), rate


class MelExtractor:
    """Holds the packed DFT table and filterbank on `device` once; ``__call__`` is one kernel launch."""

    def __init__(self, device: Union[str, torch.device] = 'cuda'):
        self.device = torch.device(device)
        self.basis = mel_filterbank(SAMPLE_RATE, N_FFT, N_MELS, FMIN, FMAX)
        self.nchunks = (live_bins(self.basis) + 15) // 16
        self.dft_tab = torch.from_numpy(pack_dft_table(self.nchunks)).to(self.device)
        self.basis_tab = torch.from_numpy(pack_basis(self.basis, self.nchunks)).to(self.device)

    def __call__(self, wav: torch.Tensor, lengths: Optional[Sequence[int]] = None, channel_last: bool = False,
                 pad_value: float = LOG_CLAMP, *, sample_rate: Optional[int] = None) -> torch.Tensor:
        """wav [B, Lmax] (or [L]) fp32 in [-1, 1] on the device, `lengths` the rows' sample counts (default: Lmax each)
        -> log-mel [B, 80, Tmax], or [B, Tmax, 80] with `channel_last`; Tmax = max(lengths) // 256, row b has
        lengths[b] // 256 frames and `pad_value` after them."""
        from .hipops import functional as HF
        if sample_rate is not None:
            check_rate(sample_rate)
        if wav.dim() == 1:
            wav = wav.unsqueeze(0)
        if wav.dim() != 2:
            raise ValueError(f"wav must be [B, L] or [L], got {tuple(wav.shape)}")
        B, Lmax = wav.shape
        lens = [Lmax] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
        if len(lens) != B:
            raise ValueError(f"{len(lens)} lengths for {B} rows")
        for i, n in enumerate(lens):
            if n < MIN_SAMPLES or n > Lmax:
                raise ValueError(f"row {i}: {n} samples outside [{MIN_SAMPLES}, {Lmax}] (reflect padding reads "
                                 f"{REFLECT} samples past each end)")
        return HF.melspec(wav, lens, self.dft_tab, self.basis_tab, self.nchunks, n_frames(max(lens)), channel_last,
                          float(pad_value))


_EXTRACTORS = {}


def extractor(device) -> MelExtractor:
    """one MelExtractor per device, built on first use."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if device not in _EXTRACTORS:
        _EXTRACTORS[device] = MelExtractor(device)
    return _EXTRACTORS[device]


def check_settings(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center) -> None:
    check_rate(sampling_rate)
    for name, got, built in (("n_fft", n_fft, N_FFT), ("num_mels", num_mels, N_MELS), ("hop_size", hop_size, HOP),
                             ("win_size", win_size, WIN), ("fmin", fmin, FMIN), ("center", bool(center), False)):
        if got != built:
            raise NotImplementedError(f"mel_spectrogram: {name}={got} (only {name}={built} is built)")
    if fmax is not None and fmax > sampling_rate / 2:
        raise NotImplementedError(f"mel_spectrogram: fmax={fmax} is above Nyquist ({sampling_rate / 2} Hz)")
    if fmax != FMAX:
        raise NotImplementedError(f"mel_spectrogram: fmax={fmax} (only fmax={FMAX} is built)")


def mel_spectrogram(y: torch.Tensor, n_fft: int = N_FFT, num_mels: int = N_MELS, sampling_rate: int = SAMPLE_RATE,
                    hop_size: int = HOP, win_size: int = WIN, fmin: float = FMIN, fmax: Optional[float] = FMAX,
                    center: bool = False) -> torch.Tensor:
    """matcha/utils/audio.py:45-82: y [B, L] on the device -> log-mel [B, num_mels, L // hop_size] fp32."""
    check_settings(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center)
    from .hipops.binding import CvftError
    if not y.is_cuda:
        raise CvftError("mel_spectrogram needs a ROCm device tensor; there is no CPU fallback")
    return extractor(y.device)(y)


# ---------------------------------------------------------------------------------
# resampling (torchaudio.transforms.Resample with its defaults: sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99)
# ---------------------------------------------------------------------------------
LOWPASS_WIDTH, ROLLOFF = 6, 0.99
RESAMPLE_TILE = 2048                          # CVFT_RESAMPLE_TILE (include/cvft.h): output samples per workgroup
RESAMPLE_MAX_TAPS = 12288                     # CVFT_RESAMPLE_MAX_TAPS: floats of the compact table, n * span
RESAMPLE_MAX_WINDOW = 16384                   # CVFT_RESAMPLE_MAX_WINDOW: floats of a tile's input window


def rate_ratio(orig: int, new: int) -> Tuple[int, int, int]:
    """(o, n, width): the rates over their gcd, and the filter's half-width in input samples."""
    orig, new = int(orig), int(new)
    if orig <= 0 or new <= 0:
        raise ValueError(f"sampling rates must be positive, got {orig} and {new}")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    return o, n, int(math.ceil(LOWPASS_WIDTH * o / (min(o, n) * ROLLOFF)))


def sinc_kernel(orig: int, new: int) -> Tuple[np.ndarray, int, int, int]:
    """-> (K fp32 [n, 2 width + o], width, o, n): K[i][k] = sinc(pi t) cos^2(pi t / 12) base / o with
    t = (-i / n + (k - width) / o) base clamped to [-6, 6] and base = 0.99 min(o, n); fp64, rounded once."""
    o, n, width = rate_ratio(orig, new)
    base = min(o, n) * ROLLOFF
    i = np.arange(n, dtype=np.float64).reshape(-1, 1)
    k = np.arange(2 * width + o, dtype=np.float64).reshape(1, -1)
    t = np.clip((-i / n + (k - width) / o) * base, -float(LOWPASS_WIDTH), float(LOWPASS_WIDTH))
    window = np.cos(np.pi * t / (2.0 * LOWPASS_WIDTH)) ** 2
    x = np.pi * t
    sinc = np.where(x == 0.0, 1.0, np.sin(x) / np.where(x == 0.0, 1.0, x))
    return (sinc * window * (base / o)).astype(np.float32), width, o, n


def compact_taps(K: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """dense K [n, cols] -> (first int32 [n], taps fp32 [n, span]): span is the longest first-to-last non-zero run of a
    row, row i keeps columns first[i] .. first[i] + span - 1 (its run, zero-padded; shifted left where it would pass the
    table's end)."""
    n, cols = K.shape
    nz = K != 0
    lo = np.where(nz.any(axis=1), nz.argmax(axis=1), 0)
    hi = np.where(nz.any(axis=1), cols - 1 - nz[:, ::-1].argmax(axis=1), 0)
    span = int((hi - lo).max()) + 1
    first = np.minimum(lo, cols - span).astype(np.int32)
    taps = K[np.arange(n)[:, None], first[:, None] + np.arange(span)[None, :]]
    return first, np.ascontiguousarray(taps.astype(np.float32))


def resampled_length(length: int, orig: int, new: int) -> int:
    """ceil(new * length / orig): the samples a `length`-sample row resamples to."""
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    return (n * int(length) + o - 1) // o


def _tile_window(o: int, n: int, width: int) -> int:
    """padded input samples the outputs of one tile can read (csrc/resample.hip: rs_window)."""
    return ((RESAMPLE_TILE - 1) // n + 2) * o + 2 * width


class Resampler:
    """`orig` Hz -> `new` Hz.  Holds the compact tap table on `device` once; ``__call__`` is one kernel launch."""

    def __init__(self, orig: int, new: int, device: Union[str, torch.device] = 'cuda'):
        self.orig, self.new, self.device = int(orig), int(new), torch.device(device)
        self.o, self.n, self.width = rate_ratio(orig, new)
        self.span, self.first, self.taps = 0, None, None
        if self.orig == self.new:
            return
        refuse = lambda what: NotImplementedError(                                                     # noqa: E731
            f"resampling {self.orig} Hz -> {self.new} Hz: {what} (o = {self.o}, n = {self.n} after the gcd)")
        # a row's run covers |t| < 6, an interval 12 o / base > 2 width - 2 columns long that holds at least 2 width - 3 of
        # them: refuse before building a huge dense table
        if self.n * (2 * self.width - 3) > RESAMPLE_MAX_TAPS:
            raise refuse(f"the tap table needs more than n * (2 width - 3) = {self.n * (2 * self.width - 3)} floats, "
                         f"the kernel holds {RESAMPLE_MAX_TAPS}")
        if _tile_window(self.o, self.n, self.width) > RESAMPLE_MAX_WINDOW:
            raise refuse(f"a tile reads {_tile_window(self.o, self.n, self.width)} input samples, the kernel holds "
                         f"{RESAMPLE_MAX_WINDOW}")
        first, taps = compact_taps(sinc_kernel(orig, new)[0])
        self.span = int(taps.shape[1])
        if self.n * self.span > RESAMPLE_MAX_TAPS:
            raise refuse(f"the tap table is n * span = {self.n * self.span} floats, the kernel holds {RESAMPLE_MAX_TAPS}")
        self.first, self.taps = torch.from_numpy(first).to(self.device), torch.from_numpy(taps).to(self.device)

    def __call__(self, wav: torch.Tensor, lengths: Optional[Sequence[int]] = None):
        """wav [B, Lmax] (or [L]) fp32 on the device, `lengths` the rows' sample counts (default: Lmax each) ->
        (out [B, Mmax] fp32, out_lengths): row b holds out_lengths[b] = ceil(new lengths[b] / orig) samples and zeros
        after them, Mmax = max(out_lengths).  With orig == new the input and `lengths` come back untouched."""
        from .hipops import functional as HF
        if self.orig == self.new:
            return wav, lengths
        if wav.dim() == 1:
            wav = wav.unsqueeze(0)
        if wav.dim() != 2:
            raise ValueError(f"wav must be [B, L] or [L], got {tuple(wav.shape)}")
        B, Lmax = wav.shape
        lens = [Lmax] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
        if len(lens) != B:
            raise ValueError(f"{len(lens)} lengths for {B} rows")
        for i, v in enumerate(lens):
            if v < 1 or v > Lmax:
                raise ValueError(f"row {i}: {v} samples outside [1, {Lmax}]")
        out_lens = [resampled_length(v, self.orig, self.new) for v in lens]
        out = HF.resample(wav, lens, self.o, self.n, self.width, self.span, self.first, self.taps, max(out_lens))
        return out, out_lens


_RESAMPLERS = {}


def resampler(orig: int, new: int, device) -> Resampler:
    """one Resampler per (orig, new, device), built on first use."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (int(orig), int(new), device)
    if key not in _RESAMPLERS:
        _RESAMPLERS[key] = Resampler(orig, new, device)
    return _RESAMPLERS[key]


def resample(wav: torch.Tensor, orig: int, new: int, lengths: Optional[Sequence[int]] = None):
    """wav [B, L] or [L] on the device at `orig` Hz -> (out [B, Mmax] at `new` Hz, out_lengths); see Resampler."""
    if int(orig) == int(new):
        return wav, lengths
    from .hipops.binding import CvftError
    if not wav.is_cuda:
        raise CvftError("resample needs a ROCm device tensor; there is no CPU fallback")
    return resampler(orig, new, wav.device)(wav, lengths)


# ---------------------------------------------------------------------------------
# the 16 kHz front-ends (cosyvoice/cli/frontend.py:131-152): whisper.log_mel_spectrogram(speech, n_mels=128) for the speech
# tokenizer, torchaudio's kaldi.fbank(speech, num_mel_bins=80, dither=0, sample_frequency=16000) for the speaker encoder
# ---------------------------------------------------------------------------------
FRONTEND_RATE = 16000
FRONT_FRAME, FRONT_HOP, FRONT_TILE = 400, 160, 64          # CVFT_FEAT16K_FRAME / _HOP / _TILE (include/cvft.h)
FRONT_STEPS = FRONT_FRAME // 16
KIND_WHISPER, KIND_FBANK = 0, 1                            # CVFT_FEAT16K_WHISPER / _FBANK
WHISPER_MELS, WHISPER_BINS, WHISPER_CHUNKS = 128, 201, 13
WHISPER_MIN_SAMPLES, WHISPER_MAX_SAMPLES = 201, 30 * FRONTEND_RATE      # reflect padding; the reference's 30 s assertion
FBANK_MELS, FBANK_NFFT, FBANK_BINS, FBANK_CHUNKS = 80, 512, 257, 16
FBANK_MIN_SAMPLES = FRONT_FRAME
FBANK_LOW_HZ, FBANK_PREEMPH, FBANK_EPS = 20.0, 0.97, 1.1920929e-07


def whisper_frames(length: int) -> int:
    """frames of the whisper log-mel: the STFT of the reflect-padded row has length // 160 + 1, the last is dropped."""
    return int(length) // FRONT_HOP


def fbank_frames(length: int) -> int:
    """frames of the kaldi fbank (snip_edges): 1 + (length - 400) // 160."""
    return 1 + (int(length) - FRONT_FRAME) // FRONT_HOP


def whisper_mel_banks() -> np.ndarray:
    """[128, 201] fp32: the Slaney bank of mel_filterbank at 16 kHz / 400 / 128 bands / 0 .. 8000 Hz -- the formula whisper's
    stored asset was made with, restated; not a copy of that asset."""
    return mel_filterbank(FRONTEND_RATE, FRONT_FRAME, WHISPER_MELS, 0.0, 8000.0)


def kaldi_mel_banks() -> np.ndarray:
    """[80, 257] fp32: torchaudio's get_mel_banks(80, 512, 16000, 20, 0, ...) restated in fp64 and rounded once.
    mel(f) = 1127 ln(1 + f / 700); 82 edges equally spaced from mel(20) to mel(8000); band b's weight at bin i < 256
    (f = 31.25 i) is max(0, min((m - left) / (center - left), (right - m) / (right - center))); no area normalisation;
    column 256 is zero."""
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)                   # noqa: E731
    edges = np.linspace(float(mel(FBANK_LOW_HZ)), float(mel(FRONTEND_RATE / 2.0)), FBANK_MELS + 2)
    left, center, right = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    m = mel(FRONTEND_RATE / FBANK_NFFT * np.arange(FBANK_NFFT // 2))[None, :]
    w = np.zeros((FBANK_MELS, FBANK_BINS), dtype=np.float64)
    w[:, :FBANK_NFFT // 2] = np.maximum(0.0, np.minimum((m - left) / (center - left), (right - m) / (right - center)))
    return w.astype(np.float32)


def whisper_dft() -> Tuple[np.ndarray, np.ndarray]:
    """(cos, sin) fp64 [201, 400]: hann[n] * cos | sin(2 pi (n k mod 400) / 400) with the periodic Hann window."""
    n = np.arange(FRONT_FRAME)
    k = np.arange(WHISPER_BINS).reshape(-1, 1)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / FRONT_FRAME)
    ang = 2.0 * np.pi * ((n * k) % FRONT_FRAME) / FRONT_FRAME
    return hann * np.cos(ang), hann * np.sin(ang)


def fbank_dft() -> Tuple[np.ndarray, np.ndarray]:
    """(cos, sin) fp64 [257, 400]: the 512-point DFT of the zero-padded frame after mean removal, pre-emphasis and the Povey
    window, as one matrix on the raw frame: D . diag(w) . P . (I - 11^T / 400).  All three steps are linear in the frame,
    so the cancellations (the frame's mean, x[n] - 0.97 x[n - 1]) happen here in fp64 rather than in fp32 on the samples."""
    n = np.arange(FRONT_FRAME)
    k = np.arange(FBANK_BINS).reshape(-1, 1)
    povey = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / (FRONT_FRAME - 1))) ** 0.85
    pre = np.eye(FRONT_FRAME) - FBANK_PREEMPH * np.eye(FRONT_FRAME, k=-1)
    pre[0, 0] -= FBANK_PREEMPH                                         # y[0] = x[0] - 0.97 x[0]
    lin = povey[:, None] * (pre @ (np.eye(FRONT_FRAME) - 1.0 / FRONT_FRAME))
    ang = 2.0 * np.pi * ((n * k) % FBANK_NFFT) / FBANK_NFFT
    return np.cos(ang) @ lin, np.sin(ang) @ lin


def pack_frame_dft(cos: np.ndarray, sin: np.ndarray, nchunks: int, live: Optional[np.ndarray] = None) -> np.ndarray:
    """the DFT operand of cvft_feat16k (include/cvft.h): dense fp64 [bins, 400] tables rounded once,
    [chunk][step][cos | sin][lane][e] with k = 16 c + (l & 15), n = 16 s + 4 (l >> 4) + e; zero for bins past the table
    and for bins where `live` (bool [bins]) is false."""
    nbin = cos.shape[0]
    full = np.zeros((2, 16 * nchunks, FRONT_FRAME), dtype=np.float32)
    keep = np.ones(nbin, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    m = min(nbin, 16 * nchunks)
    full[0, :m] = np.where(keep[:m, None], cos[:m], 0.0)
    full[1, :m] = np.where(keep[:m, None], sin[:m], 0.0)
    c = np.arange(nchunks).reshape(-1, 1, 1, 1, 1)
    s = np.arange(FRONT_STEPS).reshape(1, -1, 1, 1, 1)
    cs = np.arange(2).reshape(1, 1, -1, 1, 1)
    lane = np.arange(64).reshape(1, 1, 1, -1, 1)
    e = np.arange(4).reshape(1, 1, 1, 1, -1)
    return np.ascontiguousarray(full[cs, 16 * c + (lane & 15), 16 * s + 4 * (lane >> 4) + e])   # [nchunks, 25, 2, 64, 4]


def _rows(wav: torch.Tensor, lengths, lo: int, hi: Optional[int], what: str):
    if wav.dim() == 1:
        wav = wav.unsqueeze(0)
    if wav.dim() != 2:
        raise ValueError(f"wav must be [B, L] or [L], got {tuple(wav.shape)}")
    B, Lmax = wav.shape
    lens = [Lmax] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
    if len(lens) != B:
        raise ValueError(f"{len(lens)} lengths for {B} rows")
    top = Lmax if hi is None else min(Lmax, hi)
    for i, n in enumerate(lens):
        if n < lo or n > top:
            raise ValueError(f"row {i}: {n} samples outside [{lo}, {top}] ({what})")
    return wav, lens


class WhisperMelExtractor:
    """The speech tokenizer's input.  Holds the packed tables on `device` once; ``__call__`` is two kernel launches."""

    def __init__(self, device: Union[str, torch.device] = 'cuda'):
        self.device = torch.device(device)
        self.basis = whisper_mel_banks()
        self.nchunks = WHISPER_CHUNKS
        self.dft_tab = torch.from_numpy(pack_frame_dft(*whisper_dft(), self.nchunks)).to(self.device)
        self.basis_tab = torch.from_numpy(pack_basis(self.basis, self.nchunks)).to(self.device)

    @staticmethod
    def rows(wav: torch.Tensor, lengths):
        """-> (wav [B, Lmax], lengths); ValueError naming the row whose length is outside [201, 480000]."""
        return _rows(wav, lengths, WHISPER_MIN_SAMPLES, WHISPER_MAX_SAMPLES,
                     "reflect padding reads 200 samples past each end; the tokenizer takes at most 30 s")

    def __call__(self, wav: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
        """wav [B, Lmax] (or [L]) fp32 at 16 kHz on the device -> [B, 128, Tmax]: row b has lengths[b] // 160 frames of
        (max(log10(max(mel, 1e-10)), rowmax - 8) + 4) / 4 and 0 after them."""
        from .hipops import functional as HF
        wav, lens = self.rows(wav, lengths)
        return HF.feat16k(KIND_WHISPER, wav, lens, self.dft_tab, self.basis_tab, self.nchunks, whisper_frames(max(lens)))


class FbankExtractor:
    """The speaker encoder's input.  Holds the packed tables on `device` once; ``__call__`` is two kernel launches (one
    with ``cmn=False``)."""

    def __init__(self, device: Union[str, torch.device] = 'cuda'):
        self.device = torch.device(device)
        self.basis = kaldi_mel_banks()
        self.nchunks = FBANK_CHUNKS
        live = self.basis.any(axis=0)                                       # bins 1 .. 255
        self.dft_tab = torch.from_numpy(pack_frame_dft(*fbank_dft(), self.nchunks, live)).to(self.device)
        self.basis_tab = torch.from_numpy(pack_basis(self.basis, self.nchunks)).to(self.device)

    @staticmethod
    def rows(wav: torch.Tensor, lengths):
        """-> (wav [B, Lmax], lengths); ValueError naming the row that is shorter than one frame of 400 samples."""
        return _rows(wav, lengths, FBANK_MIN_SAMPLES, None, "a frame is 400 samples, snip_edges")

    def __call__(self, wav: torch.Tensor, lengths: Optional[Sequence[int]] = None, cmn: bool = True) -> torch.Tensor:
        """wav [B, Lmax] (or [L]) fp32 in [-1, 1] at 16 kHz on the device -> [B, Mmax, 80]: row b has
        1 + (lengths[b] - 400) // 160 frames of log(max(energy, 2^-23)), minus each band's mean over them with `cmn`, and
        0 after them."""
        from .hipops import functional as HF
        wav, lens = self.rows(wav, lengths)
        return HF.feat16k(KIND_FBANK, wav, lens, self.dft_tab, self.basis_tab, self.nchunks, fbank_frames(max(lens)),
                          finish=bool(cmn))


_FRONT_EXTRACTORS = {}


def _front_extractor(cls, device):
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if (cls, device) not in _FRONT_EXTRACTORS:
        _FRONT_EXTRACTORS[(cls, device)] = cls(device)
    return _FRONT_EXTRACTORS[(cls, device)]


def whisper_extractor(device) -> WhisperMelExtractor:
    """one WhisperMelExtractor per device, built on first use."""
    return _front_extractor(WhisperMelExtractor, device)


def fbank_extractor(device) -> FbankExtractor:
    """one FbankExtractor per device, built on first use."""
    return _front_extractor(FbankExtractor, device)


def whisper_log_mel(wav: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    """whisper.log_mel_spectrogram(wav, n_mels=128) per row: wav [B, L] or [L] at 16 kHz on the device -> [B, 128, Tmax]."""
    from .hipops.binding import CvftError
    WhisperMelExtractor.rows(wav, lengths)                                  # length errors come first, device or not
    if not wav.is_cuda:
        raise CvftError("whisper_log_mel needs a ROCm device tensor; there is no CPU fallback")
    return whisper_extractor(wav.device)(wav, lengths)


def kaldi_fbank(wav: torch.Tensor, lengths: Optional[Sequence[int]] = None, cmn: bool = True) -> torch.Tensor:
    """kaldi.fbank(wav, num_mel_bins=80, dither=0, sample_frequency=16000) per row, minus its mean over the row's frames
    with `cmn`: wav [B, L] or [L] at 16 kHz on the device -> [B, Mmax, 80]."""
    from .hipops.binding import CvftError
    FbankExtractor.rows(wav, lengths)
    if not wav.is_cuda:
        raise CvftError("kaldi_fbank needs a ROCm device tensor; there is no CPU fallback")
    return fbank_extractor(wav.device)(wav, lengths, cmn)
