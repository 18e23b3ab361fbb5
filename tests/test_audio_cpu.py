"""The mel front-end's host side (no GPU): the Slaney filterbank's anchors, the reference math restated in fp64 against
the reference's own mels (tests/golden/melspec.npz, tools/make_golden_melspec.py), the table packing the kernel reads,
load_wav, prepare_joint_data's manifest handling and the settings that are not built."""
import json
import math
import os

import numpy as np
import pytest
import torch

import audio_fixtures as AF
from cosyvoice_lora_finetune_framework_amd import audio as A

SETTING = dict(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000, center=False)


@pytest.fixture(scope="module")
def gold():
    return AF.load()


def test_mel_filterbank_anchors(gold):
    """Peak rule: a row's largest sample is at the bin nearest its centre frequency -- except that above 1 kHz a
    triangle's falling side is exp(ln(6.4)/27 * 0.552 mel) = 1.039 times as long as its rising side, which moves the
    tie between the two neighbouring bins from a fractional position of 0.5 to 1 / 2.039 = 0.4907: a centre within
    0.01 bin of half-way may peak at either neighbour (band 34, centre at bin 63.4987, does)."""
    b = A.mel_filterbank(22050, 1024, 80, 0, 8000)
    assert b.shape == (80, 513) and b.dtype == np.float32
    assert float(A.hz_to_mel(1000)) == 15
    assert float(A.hz_to_mel(8000)) == 15 + 27 * math.log(8) / math.log(6.4)
    assert (b >= 0).all() and (b.sum(axis=1) > 0).all()
    assert A.live_bins(b) - 1 == 371 and not b[:, 372:].any() and b[:, 371].any()
    centre = A.mel_frequencies(82, 0, 8000)[1:-1] * 1024 / 22050
    peak = b.argmax(axis=1)
    for i in range(80):
        if abs(centre[i] - math.floor(centre[i]) - 0.5) < 0.01:
            assert peak[i] in (math.floor(centre[i]), math.ceil(centre[i])), i
        else:
            assert peak[i] == round(centre[i]), (i, centre[i], peak[i])
    area = b.astype(np.float64).sum(axis=1) * 22050 / 1024
    assert np.abs(area - 1).max() < 0.10, area
    assert b.tobytes() == gold[2].tobytes()


def test_reference_math_in_fp64_reproduces_the_golden_mels(gold):
    wavs, mels, _, meta = gold
    basis = A.mel_filterbank(22050, 1024, 80, 0, 8000)
    for L in AF.LENGTHS:
        err = np.abs(AF.mel_fp64(wavs[L], basis) - mels[L]).max()
        print(L, "fp64 restatement vs reference", err)
        assert err <= 1e-5, (L, err)
    assert float(np.float32(A.LOG_CLAMP)) == float(np.log(np.float32(1e-5)))
    assert meta["cases"]["2660"]["silent_frames"] >= 1 and meta["cases"]["22050"]["silent_frames"] >= 1


def test_frame_count_rule(gold):
    wavs, mels, _, _ = gold
    for L in AF.LENGTHS:
        assert wavs[L].shape == (L,) and mels[L].shape == (80, L // 256) and A.n_frames(L) == L // 256
        assert AF.frames_of(wavs[L]).shape == (L // 256, 1024)
        assert (L + 2 * A.REFLECT - A.N_FFT) // A.HOP + 1 == L // 256


def test_packed_tables_hold_the_dft_and_the_basis():
    """unpack what the kernel reads (include/cvft.h, cvft_melspec) and compare with the plain matrices; every (bin, n)
    pair and every (band, bin) pair appears exactly once."""
    basis = A.mel_filterbank(22050, 1024, 80, 0, 8000)
    nch = (A.live_bins(basis) + 15) // 16
    assert nch == 24
    tab = A.pack_dft_table(nch).astype(np.float64)
    n = np.arange(1024)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * n / 1024)
    seen = np.zeros((16 * nch, 1024), dtype=np.int64)
    for c in (0, 7, nch - 1):
        for lane in range(64):
            k = 16 * c + (lane & 15)
            for s in range(64):
                ns = 256 * (s >> 4) + 64 * (lane >> 4) + 4 * (s & 15) + np.arange(4)
                seen[k, ns] += 1
                assert np.abs(tab[c, s, 0, lane] - hann[ns] * np.cos(2 * np.pi * k * ns / 1024)).max() < 1e-7
                assert np.abs(tab[c, s, 1, lane] - hann[ns] * np.sin(2 * np.pi * k * ns / 1024)).max() < 1e-7
        assert (seen[16 * c:16 * c + 16] == 1).all()
    pb = A.pack_basis(basis, nch)
    assert pb.shape == (nch, 5, 64, 4)
    full = np.zeros((80, 16 * nch), dtype=np.float32)
    for c in range(nch):
        for m in range(5):
            for lane in range(64):
                full[16 * m + (lane & 15), 16 * c + 4 * (lane >> 4):16 * c + 4 * (lane >> 4) + 4] = pb[c, m, lane]
    assert np.array_equal(full[:, :372], basis[:, :372]) and not full[:, 372:].any()


def test_load_wav_round_trips_write_wav(tmp_path, gold):
    from cosyvoice_lora_finetune_framework_amd.inference_joint import pcm16, write_wav
    x = torch.from_numpy(gold[0][2660])
    write_wav(str(tmp_path / "a.wav"), x)
    y, rate = A.load_wav(str(tmp_path / "a.wav"))
    assert rate == 22050 and y.dtype == torch.float32 and y.shape == x.shape
    assert np.array_equal(y.numpy(), pcm16(x).astype(np.float32) / 32768.0)
    assert float((y - x).abs().max()) <= 1.0 / 32768
    write_wav(str(tmp_path / "b.wav"), x, rate=16000)
    assert A.load_wav(str(tmp_path / "b.wav"))[1] == 16000
    with pytest.raises(NotImplementedError, match="16000"):
        A.check_rate(16000)


def _manifest(tmp_path, gold, lengths):
    from cosyvoice_lora_finetune_framework_amd.inference_joint import write_wav
    lines = []
    for i, L in enumerate(lengths):
        x = torch.from_numpy(gold[0][22050]).repeat(1 + L // 22050)[:L]
        write_wav(str(tmp_path / f"u{i}.wav"), x)
        lines.append(dict(utt=f"u{i}", wav=f"u{i}.wav", text=f"text {i}", text_token=[3 + i, 4], speech_token=[5, 6, 7 + i],
                          utt_embedding=[0.01 * j for j in range(192)]))
    path = tmp_path / "m.jsonl"
    path.write_text("\n".join(json.dumps(e) for e in lines) + "\n\n")
    return path, lines


def test_prepare_joint_data_manifest_and_duration_filter(tmp_path, gold):
    from cosyvoice_lora_finetune_framework_amd import prepare_joint_data as P
    path, lines = _manifest(tmp_path, gold, [11024, 11025, 22050])          # 0.49995 s, 0.5 s, 1 s
    entries = P.read_manifest(str(path))
    assert [e["utt"] for e in entries] == ["u0", "u1", "u2"]
    assert all(os.path.isabs(e["wav"]) and os.path.exists(e["wav"]) for e in entries)
    assert P.wav_info(entries[0]["wav"]) == (11024, 22050)
    assert [e["utt"] for e in P.filter_entries(entries, verbose=False)] == ["u1", "u2"]
    assert P.keep_duration(11025, 22050) and P.keep_duration(30 * 22050, 22050)
    assert not P.keep_duration(11024, 22050) and not P.keep_duration(30 * 22050 + 1, 22050)
    bad = tmp_path / "bad.jsonl"
    bad.write_text(json.dumps({k: v for k, v in lines[0].items() if k != "speech_token"}) + "\n")
    with pytest.raises(ValueError, match="speech_token"):
        P.read_manifest(str(bad))
    row = P.make_row(entries[2], torch.arange(160.0).reshape(2, 80))
    assert tuple(row) == P.COLUMNS and row["speech_feat_shape"] == [2, 80] and len(row["speech_feat"]) == 160
    assert row["spk_embedding"] == row["utt_embedding"] and len(row["utt_embedding"]) == 192


@pytest.mark.parametrize("change", [dict(n_fft=2048), dict(hop_size=320), dict(win_size=800), dict(center=True),
                                    dict(num_mels=128), dict(fmin=50), dict(fmax=12000), dict(fmax=7600),
                                    dict(fmax=None), dict(sampling_rate=24000)])
def test_out_of_scope_settings_raise(change):
    kw = dict(SETTING, **change)
    name = "sampling rate" if "sampling_rate" in change else next(iter(change))
    with pytest.raises(NotImplementedError, match=name):
        A.mel_spectrogram(torch.zeros(1, 4096), **kw)
