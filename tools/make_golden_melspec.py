#!/usr/bin/env python3
"""Golden vectors for the mel front-end (tests/golden/melspec.npz, melspec_meta.json).

Runs the REFERENCE's own ``matcha/utils/audio.py: mel_spectrogram`` on the CPU at the CosyVoice-300M setting
(1024, 80, 22050, 256, 1024, 0, 8000, center=False).  The file is loaded by path, because its package ``__init__``
imports hydra; ``librosa.filters.mel``, which is not installed, is stood in for by ``audio.mel_filterbank`` (a
restatement of librosa's documented formula), so the stored basis is this project's.

The signals are ``tests/audio_fixtures.make_wave``.  A case is only written when the reference's fp32 output and the
fp64 restatement of the same math (``audio_fixtures.mel_fp64``) agree to <= 1e-5 -- a signal on which torch's own FFT is
ill-conditioned would fail that -- and when between 5 % and 40 % of the frames of the L = 2660 and L = 22050 cases
contain clamped bands.

usage: CVFT_REFERENCE=<reference>/cosyvoice_flow_finetune python tools/make_golden_melspec.py
"""
import importlib.util
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from audio_fixtures import GOLD, LENGTHS, SEEDS, make_wave, mel_fp64  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.audio import mel_filterbank  # noqa: E402


def reference_module():
    root = os.environ.get("CVFT_REFERENCE")
    if not root:
        raise SystemExit("set CVFT_REFERENCE to the reference's cosyvoice_flow_finetune directory")
    librosa, filters = types.ModuleType("librosa"), types.ModuleType("librosa.filters")
    filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    librosa.filters = filters
    sys.modules.setdefault("librosa", librosa)
    sys.modules.setdefault("librosa.filters", filters)
    spec = importlib.util.spec_from_file_location("ref_matcha_audio", os.path.join(root, "matcha", "utils", "audio.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = reference_module()
    basis = mel_filterbank(22050, 1024, 80, 0, 8000)
    arrays, meta = dict(basis=basis), dict(setting=[1024, 80, 22050, 256, 1024, 0, 8000], cases={})
    for L in LENGTHS:
        wav = make_wave(L, SEEDS[L])
        with torch.no_grad():
            mel = ref.mel_spectrogram(torch.from_numpy(wav)[None], 1024, 80, 22050, 256, 1024, 0, 8000, center=False)[0].numpy()
        assert mel.shape == (80, L // 256), mel.shape
        err = float(np.abs(mel.astype(np.float64) - mel_fp64(wav, basis)).max())
        floor = np.log(np.float32(1e-5))
        clamped = float((mel == floor).any(axis=0).mean())
        silent = int((mel == floor).all(axis=0).sum())
        assert err <= 1e-5, f"L={L}: reference fp32 vs fp64 restatement {err}"
        if L in (2660, 22050):
            assert 0.05 <= clamped <= 0.40, f"L={L}: {clamped} of the frames contain clamped bands"
        arrays[f"wav_{L}"], arrays[f"mel_{L}"] = wav, mel
        meta["cases"][str(L)] = dict(L=L, T=L // 256, seed=SEEDS[L], ref_vs_fp64=err, clamped_frame_fraction=clamped,
                                     silent_frames=silent, peak=float(np.abs(wav).max()))
        print(L, meta["cases"][str(L)])
    assert torch.equal(ref.mel_basis[next(iter(ref.mel_basis))], torch.from_numpy(basis))
    np.savez_compressed(os.path.join(GOLD, "melspec.npz"), **arrays)
    with open(os.path.join(GOLD, "melspec_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("bytes", os.path.getsize(os.path.join(GOLD, "melspec.npz")))


if __name__ == "__main__":
    main()
