"""The resampler's host side against the fp64 restatement (tests/resample_fixtures.py): the tap table, its compact form,
output lengths, the restatement itself on a sine, the refusals, and load_wav's sample widths."""
import math
import wave

import numpy as np
import pytest
import torch

import resample_fixtures as RF
from cosyvoice_lora_finetune_framework_amd import audio as A

WIDTHS = {(16000, 22050): (7, 320, 441), (24000, 22050): (7, 160, 147), (44100, 22050): (13, 2, 1),
          (48000, 22050): (14, 320, 147), (22050, 16000): (9, 441, 320), (22050, 48000): (7, 147, 320)}


@pytest.mark.parametrize("pair", RF.PAIRS)
def test_tap_table_is_the_formula(pair):
    K, width, o, n = A.sinc_kernel(*pair)
    want = RF.dense_table(*pair)
    assert K.dtype == np.float32 and K.shape == (n, 2 * width + o) == want.shape
    assert np.array_equal(K.view(np.uint32), want.view(np.uint32))
    r = RF.ratio(*pair)
    assert (width, o, n) == WIDTHS[pair] == (r[2], r[0], r[1])
    # DC gain: every phase's taps sum to 1, so a constant input resamples to the same constant away from the edges
    sums = K.astype(np.float64).sum(axis=1)
    assert float(np.abs(sums - 1.0).max()) <= 1e-3, sums
    L = 3001
    y = RF.resample_fp64(np.ones(L, dtype=np.float32), *pair)
    edge = 2 * width * n // o + 2
    assert float(np.abs(y[edge:-edge] - 1.0).max()) <= 1e-3


@pytest.mark.parametrize("pair", RF.PAIRS + [(32000, 22050)])
def test_compaction_round_trips(pair):
    K, width, o, n = A.sinc_kernel(*pair)
    first, taps = A.compact_taps(K)
    span = taps.shape[1]
    assert first.dtype == np.int32 and taps.dtype == np.float32 and first.shape == (n,) and taps.shape == (n, span)
    assert 1 <= span <= 2 * width + 1 and span == RF.longest_run(K)
    if pair in RF.SPANS:
        assert span == RF.SPANS[pair]
    assert int(first.min()) >= 0 and int(first.max()) + span <= K.shape[1]
    dense = np.zeros_like(K)
    for i in range(n):
        dense[i, first[i]:first[i] + span] = taps[i]
    assert np.array_equal(dense, K)                     # by value: the dense table's zeros outside a run may be -0.0
    assert n * span <= A.RESAMPLE_MAX_TAPS and A.RESAMPLE_MAX_TAPS * 4 >= 32 * 1024


@pytest.mark.parametrize("pair", RF.PAIRS)
def test_resampled_length_is_the_ceiling(pair):
    o, n = RF.ratio(*pair)[:2]
    for L in (1, o - 1, o, o + 1, 3001):
        M = A.resampled_length(L, *pair)
        assert M * o >= n * L > (M - 1) * o, (pair, L, M)
        assert M == RF.out_length(L, *pair)


@pytest.mark.parametrize("pair", RF.PAIRS)
def test_restatement_resamples_a_sine(pair):
    orig, new = pair
    o, n, width, _ = RF.ratio(*pair)
    L = 3001
    x = np.sin(2.0 * np.pi * 1000.0 * np.arange(L) / orig)
    y = RF.resample_fp64(x, orig, new)
    assert y.shape == (RF.out_length(L, orig, new),)
    want = np.sin(2.0 * np.pi * 1000.0 * np.arange(y.shape[0]) / new)
    edge = 2 * width * n // o + 2
    err = float(np.abs(y - want)[edge:-edge].max())
    print(f"{orig} -> {new}: max |restatement - analytic sine| = {err:.2e}")
    assert err <= 1e-3


def test_refusals():
    with pytest.raises(NotImplementedError, match="16000"):
        A.check_rate(16000)
    with pytest.raises(NotImplementedError, match="sampling rate"):
        A.mel_spectrogram(torch.zeros(1, 4096), sampling_rate=16000)
    with pytest.raises(NotImplementedError, match=r"22050 Hz -> 22051 Hz"):
        A.Resampler(22050, 22051, "cpu")
    with pytest.raises(NotImplementedError, match=r"96000 Hz -> 8000 Hz"):
        A.Resampler(96000, 8000, "cpu")                     # a tile's input window: o / n = 12
    x = torch.zeros(4)
    same = A.Resampler(22050, 22050, "cpu")
    assert same(x)[0] is x and same(x, [3]) == (x, [3]) and A.resample(x, 16000, 16000)[0] is x


def _write(path, width, rate, frames: bytes, channels=1):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(frames)


def test_load_wav_reads_8_16_24_and_32_bit_pcm(tmp_path):
    from cosyvoice_lora_finetune_framework_amd.inference_joint import pcm16, write_wav
    v8 = np.array([0, 1, 127, 128, 129, 255], dtype=np.uint8)
    _write(tmp_path / "a8.wav", 1, 8000, v8.tobytes())
    x, rate = A.load_wav(str(tmp_path / "a8.wav"))
    assert rate == 8000 and x.dtype == torch.float32
    assert x.tolist() == [-1.0, -127 / 128, -1 / 128, 0.0, 1 / 128, 127 / 128]

    v24 = [0, 1, -1, 2 ** 23 - 1, -2 ** 23, 0x123456, -0x123456, 256, -65536]
    _write(tmp_path / "a24.wav", 3, 48000, b"".join(int(v).to_bytes(3, "little", signed=True) for v in v24))
    x, rate = A.load_wav(str(tmp_path / "a24.wav"))
    assert rate == 48000 and x.dtype == torch.float32
    assert x.tolist() == [v / 2.0 ** 23 for v in v24]                     # 24-bit values are exact in fp32

    v32 = np.array([0, 1, -1, 2 ** 31 - 1, -2 ** 31, 0x12345678, -0x12345678, 1 << 20], dtype="<i4")
    _write(tmp_path / "a32.wav", 4, 44100, v32.tobytes())
    x, rate = A.load_wav(str(tmp_path / "a32.wav"))
    assert rate == 44100 and x.dtype == torch.float32
    assert np.array_equal(x.numpy(), (v32.astype(np.float64) / 2.0 ** 31).astype(np.float32))
    assert float(x.min()) == -1.0 and float(x.abs().max()) <= 1.0

    st = np.array([[100, 300], [-32768, 32767]], dtype="<i2")              # two channels are averaged, as before
    _write(tmp_path / "st.wav", 2, 22050, st.tobytes(), channels=2)
    x, _ = A.load_wav(str(tmp_path / "st.wav"))
    assert np.array_equal(x.numpy(), (st.astype(np.float32) / 32768.0).mean(axis=1, dtype=np.float32))

    w = torch.from_numpy(RF.noise(999, 3))
    write_wav(str(tmp_path / "a16.wav"), w)
    x, rate = A.load_wav(str(tmp_path / "a16.wav"))
    assert rate == 22050 and np.array_equal(x.numpy(), pcm16(w).astype(np.float32) / 32768.0)
