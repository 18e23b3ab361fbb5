"""The host side of the 16 kHz front-ends (audio.whisper_log_mel / audio.kaldi_fbank) without a GPU:
the two filterbanks, frame counts, the packed tables the kernel reads, length errors, the manifest rules of
prepare_joint_data with and without the model hooks, the onnxruntime error, and the yardstick itself -- the fp32 restatement
of tests/feat16k_fixtures.py stays within the caps the GPU tests rely on."""
import json
import sys

import numpy as np
import pytest
import torch

import feat16k_fixtures as FX
from cosyvoice_lora_finetune_framework_amd import audio as A


def test_kaldi_bank():
    bank = A.kaldi_mel_banks()
    assert bank.shape == (80, 257) and bank.dtype == np.float32
    assert bank.min() >= 0.0 and bank.max() <= 1.0
    assert not bank[:, 0].any() and not bank[:, 256].any()
    first = np.flatnonzero(bank[0])[0]
    assert first * 16000 / 512 > 20.0                                   # band 0 starts above 20 Hz
    assert bank.any(axis=1).all()                                       # every band has a non-zero bin
    assert bank[:, 1:256].any(axis=0).all()                             # bins 1 .. 255 are the live ones
    # the independent restatement of the fixtures: the same formula written another way, so a rounding apart at most
    assert np.abs(bank.astype(np.float64) - FX.kaldi_bank().astype(np.float64)).max() <= 2.0 ** -22


def test_whisper_bank():
    bank = A.whisper_mel_banks()
    assert bank.shape == (128, 201) and bank.dtype == np.float32
    assert np.array_equal(bank, A.mel_filterbank(16000, 400, 128, 0.0, 8000.0))
    assert bank.min() >= 0.0 and bank.any(axis=1).all()


def test_frame_counts():
    assert A.FRONTEND_RATE == 16000
    for L in (201, 400, 559, 560, 720, 10400, 16000, 480000):
        assert A.whisper_frames(L) == L // 160 == FX.whisper_frames(L)
    for L in (400, 559, 560, 720, 10400, 16000):
        assert A.fbank_frames(L) == 1 + (L - 400) // 160 == FX.fbank_frames(L)
    assert (A.fbank_frames(400), A.fbank_frames(559), A.fbank_frames(560)) == (1, 1, 2)
    assert (A.whisper_frames(400), A.whisper_frames(201)) == (2, 1)
    assert (A.whisper_frames(10400), A.fbank_frames(10400)) == (65, 63)


def _unpack_dft(tab, nbins):
    """[chunk][step][cos | sin][lane][e] -> dense (cos, sin) [16 * chunks, 400], every cell visited exactly once."""
    nch = tab.shape[0]
    dense = np.full((2, 16 * nch, 400), np.nan, dtype=np.float32)
    for c in range(nch):
        for s in range(25):
            for lane in range(64):
                for e in range(4):
                    k, n = 16 * c + (lane & 15), 16 * s + 4 * (lane >> 4) + e
                    assert np.isnan(dense[0, k, n])
                    dense[:, k, n] = tab[c, s, :, lane, e]
    assert not np.isnan(dense).any()
    return dense


def test_packed_whisper_tables_unpack_to_the_dense_ones():
    cos, sin = A.whisper_dft()
    assert cos.dtype == np.float64 and cos.shape == (201, 400)
    n, k = np.arange(400.0), np.arange(201.0)[:, None]
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * n / 400)
    assert np.abs(cos - hann * np.cos(2 * np.pi * n * k / 400)).max() < 1e-12
    tab = A.pack_frame_dft(cos, sin, A.WHISPER_CHUNKS)
    assert tab.shape == (13, 25, 2, 64, 4) and tab.dtype == np.float32
    dense = _unpack_dft(tab, 201)
    assert np.array_equal(dense[0, :201], cos.astype(np.float32)) and np.array_equal(dense[1, :201], sin.astype(np.float32))
    assert not dense[:, 201:].any()
    basis = A.pack_basis(A.whisper_mel_banks(), A.WHISPER_CHUNKS)
    assert basis.shape == (13, 8, 64, 4)
    bank = A.whisper_mel_banks()
    for c, m, lane, i in ((0, 0, 0, 0), (3, 2, 37, 1), (12, 7, 63, 3), (12, 7, 15, 0)):
        b, col = 16 * m + (lane & 15), 16 * c + 4 * (lane >> 4) + i
        assert basis[c, m, lane, i] == (bank[b, col] if col < 201 else 0.0)


def test_packed_fbank_tables_fold_the_frame_steps():
    cos, sin = A.fbank_dft()
    assert cos.shape == (257, 400) and cos.dtype == np.float64
    # the folded matrix applied to a frame equals the steps applied one after another (fp64)
    x = np.random.default_rng(0).random(400) - 0.3
    y = x - x.mean()
    y = y - 0.97 * np.concatenate([y[:1], y[:-1]])
    y = y * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 399)) ** 0.85
    spec = np.fft.rfft(y, 512)
    assert np.abs(cos @ x - spec.real).max() < 1e-10 and np.abs(sin @ x + spec.imag).max() < 1e-10
    assert np.abs(cos.sum(axis=1)).max() < 1e-10                         # a constant frame gives nothing
    bank = A.kaldi_mel_banks()
    live = bank.any(axis=0)
    tab = A.pack_frame_dft(cos, sin, A.FBANK_CHUNKS, live)
    assert tab.shape == (16, 25, 2, 64, 4)
    dense = _unpack_dft(tab, 257)
    assert np.array_equal(dense[0, 1:256], cos[1:256].astype(np.float32))
    assert np.array_equal(dense[1, 1:256], sin[1:256].astype(np.float32))
    assert not dense[:, 0].any()                                         # bin 0 carries no weight
    assert A.pack_basis(bank, A.FBANK_CHUNKS).shape == (16, 5, 64, 4)


def test_length_errors_name_the_row():
    from cosyvoice_lora_finetune_framework_amd.hipops.binding import CvftError
    x = torch.zeros(2, 800)
    with pytest.raises(ValueError, match="row 1: 200 samples"):
        A.whisper_log_mel(x, [800, 200])
    with pytest.raises(ValueError, match="row 0: 399 samples"):
        A.kaldi_fbank(x, [399, 800])
    with pytest.raises(ValueError, match="row 1: 801 samples"):
        A.kaldi_fbank(x, [800, 801])
    with pytest.raises(ValueError, match="3 lengths for 2 rows"):
        A.whisper_log_mel(x, [800, 800, 800])
    with pytest.raises(ValueError, match="row 0: 480001 samples"):
        A.whisper_log_mel(torch.zeros(480001))
    with pytest.raises(CvftError, match="no CPU fallback"):               # valid lengths, but no device: no fallback
        A.whisper_log_mel(x)
    with pytest.raises(CvftError, match="no CPU fallback"):
        A.kaldi_fbank(x, [400, 800], cmn=False)


def test_manifest_validation_with_and_without_the_hooks(tmp_path):
    from cosyvoice_lora_finetune_framework_amd import prepare_joint_data as P
    full = dict(utt="a", wav="a.wav", text="t", text_token=[1, 2], speech_token=[3], utt_embedding=[0.0] * 192)
    bare = {k: v for k, v in full.items() if k not in ("speech_token", "utt_embedding")}
    path = tmp_path / "m.jsonl"
    path.write_text(json.dumps(full) + "\n" + json.dumps(dict(bare, utt="b")) + "\n")
    with pytest.raises(ValueError, match=r"m.jsonl:2: missing speech_token, utt_embedding"):
        P.read_manifest(str(path))
    with pytest.raises(ValueError, match=r"m.jsonl:2: missing utt_embedding"):
        P.read_manifest(str(path), ("speech_token",))
    with pytest.raises(ValueError, match=r"m.jsonl:2: missing speech_token"):
        P.read_manifest(str(path), ("utt_embedding",))
    entries = P.read_manifest(str(path), ("speech_token", "utt_embedding"))
    assert [e["utt"] for e in entries] == ["a", "b"] and entries[0]["speech_token"] == [3] and "speech_token" not in entries[1]
    # prepare() without the hooks reports the same missing keys as before
    with pytest.raises(ValueError, match="missing speech_token, utt_embedding"):
        P.prepare(str(path), str(tmp_path / "out"), device="cpu", verbose=False)
    path.write_text(json.dumps(dict(full, speech_token=[])) + "\n")
    with pytest.raises(ValueError, match="empty token list"):
        P.read_manifest(str(path), ("speech_token",))


def test_from_onnx_without_onnxruntime_names_it(monkeypatch):
    from cosyvoice_lora_finetune_framework_amd import frontend16k as F
    monkeypatch.setitem(sys.modules, "onnxruntime", None)                 # import onnxruntime -> ImportError
    with pytest.raises(F.OnnxRuntimeMissing, match="onnxruntime is not installed"):
        F.SpeechFrontend.from_onnx("speech_tokenizer_v1.onnx", "campplus.onnx", device="cpu")
    with pytest.raises(F.OnnxRuntimeMissing, match="campplus.onnx"):
        F.SpeechFrontend.from_onnx(None, "campplus.onnx", device="cpu")
    fe = F.SpeechFrontend("cpu")
    with pytest.raises(RuntimeError, match="no speech tokenizer"):
        fe.tokens(torch.zeros(800))
    with pytest.raises(RuntimeError, match="no speaker encoder"):
        fe.embeddings(torch.zeros(800))


@pytest.mark.parametrize("name", [n for n, _ in FX.CASES + FX.WHISPER_ONLY])
def test_fp32_restatement_stays_within_the_caps(name):
    """d_ref = max |fp32 restatement - fp64 restatement|: <= 1e-4 for the whisper log-mel (the GPU bound itself) and for the
    fbank with and without the mean (the condition under which 4 d_ref is allowed as its GPU bound)."""
    want, d = FX.reference("whisper", name)
    assert want.shape == (128, FX.whisper_frames(FX.signal(name).shape[0]))
    print(f"whisper {name}: d_ref = {d:.3e}")
    assert d <= 1e-4
    if name == "201":
        return
    for cmn in (True, False):
        want, d = FX.reference("fbank", name, cmn)
        assert want.shape == (FX.fbank_frames(FX.signal(name).shape[0]), 80)
        print(f"fbank cmn={cmn} {name}: d_ref = {d:.3e}")
        assert d <= 1e-4
    if name == "16000z":                                                 # the silent stretch sits on the floors
        raw = FX.kaldi_fbank(FX.signal(name), False, np.float32)
        assert (raw[34:44] == FX.K_FLOOR).all() and (raw[:33] > FX.K_FLOOR).all()
