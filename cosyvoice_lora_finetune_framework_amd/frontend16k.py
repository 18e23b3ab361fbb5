"""16 kHz audio -> speech tokens and speaker embeddings: the two model legs of the reference's front-end
(cosyvoice/cli/frontend.py:131-152) around features computed on the GPU.

The features -- ``audio.whisper_log_mel`` for the speech tokenizer, ``audio.kaldi_fbank`` for the speaker encoder -- run on
the device, batched and ragged (csrc/feat16k.hip).  The two models themselves are external ONNX files the reference ships
without source, so they are plain callables here:

    speech_tokenizer(feat [1, 128, T] fp32 numpy, length T) -> token ids
    speaker_encoder(feat [1, M, 80] fp32 numpy)             -> 192 floats

``SpeechFrontend.from_onnx`` builds them from ``onnxruntime`` sessions on the CPU provider, fed as the reference feeds
them.  ``onnxruntime`` is imported only there; without it ``from_onnx`` raises ``OnnxRuntimeMissing``.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import audio as A

EMBED_DIM = 192


class OnnxRuntimeMissing(ImportError):
    """onnxruntime is not installed: the ONNX speech tokenizer / speaker encoder cannot be loaded."""


def _session(path: str):
    try:
        import onnxruntime
    except ImportError as e:
        raise OnnxRuntimeMissing(f"onnxruntime is not installed, so {path} cannot be loaded; install it, or pass callables "
                                 f"to SpeechFrontend(speech_tokenizer=..., speaker_encoder=...)") from e
    opt = onnxruntime.SessionOptions()
    opt.graph_optimization_level = onnxruntime.GraphOptimizationLevel.ORT_ENABLE_ALL
    opt.intra_op_num_threads = 1
    return onnxruntime.InferenceSession(path, sess_options=opt, providers=["CPUExecutionProvider"])


def onnx_speech_tokenizer(path: str) -> Callable:
    """frontend.py:134-139: inputs [0] = the log-mel, [1] = its frame count as int32 [1]; output [0] flattened."""
    sess = _session(path)
    names = [i.name for i in sess.get_inputs()]

    def run(feat: np.ndarray, length: int) -> List[int]:
        out = sess.run(None, {names[0]: feat, names[1]: np.array([length], dtype=np.int32)})[0]
        return [int(v) for v in out.flatten().tolist()]
    return run


def onnx_speaker_encoder(path: str) -> Callable:
    """frontend.py:149-150: input [0] = the mean-subtracted fbank [1, M, 80]; output [0] flattened."""
    sess = _session(path)
    name = sess.get_inputs()[0].name

    def run(feat: np.ndarray) -> List[float]:
        return sess.run(None, {name: feat})[0].flatten().tolist()
    return run


class SpeechFrontend:
    """`speech_tokenizer` / `speaker_encoder`: the callables above, or None for a leg that is not wanted."""

    def __init__(self, device='cuda', speech_tokenizer: Optional[Callable] = None, speaker_encoder: Optional[Callable] = None):
        self.device = torch.device(device)
        self.speech_tokenizer, self.speaker_encoder = speech_tokenizer, speaker_encoder

    @classmethod
    def from_onnx(cls, tokenizer_path: Optional[str] = None, campplus_path: Optional[str] = None, device='cuda'):
        return cls(device, onnx_speech_tokenizer(tokenizer_path) if tokenizer_path else None,
                   onnx_speaker_encoder(campplus_path) if campplus_path else None)

    def _rows(self, wav16k: torch.Tensor, lengths):
        wav16k = wav16k.reshape(1, -1) if wav16k.dim() == 1 else wav16k
        lens = [wav16k.shape[1]] * wav16k.shape[0] if lengths is None else [int(v) for v in lengths]
        return wav16k.float().to(self.device), lens

    def tokens(self, wav16k: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> List[List[int]]:
        """wav16k [B, L] (or [L]) at 16 kHz -> the speech token ids of every row."""
        if self.speech_tokenizer is None:
            raise RuntimeError("no speech tokenizer was given (SpeechFrontend(speech_tokenizer=...) / --speech-tokenizer)")
        wav, lens = self._rows(wav16k, lengths)
        feat = A.whisper_log_mel(wav, lens).cpu().numpy()
        out = []
        for r, n in enumerate(lens):
            T = A.whisper_frames(n)
            out.append([int(v) for v in self.speech_tokenizer(np.ascontiguousarray(feat[r:r + 1, :, :T]), T)])
        return out

    def embeddings(self, wav16k: torch.Tensor, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
        """wav16k [B, L] (or [L]) at 16 kHz -> speaker embeddings [B, 192] fp32 (CPU)."""
        if self.speaker_encoder is None:
            raise RuntimeError("no speaker encoder was given (SpeechFrontend(speaker_encoder=...) / --campplus)")
        wav, lens = self._rows(wav16k, lengths)
        feat = A.kaldi_fbank(wav, lens, cmn=True).cpu().numpy()
        rows = []
        for r, n in enumerate(lens):
            e = np.asarray(self.speaker_encoder(np.ascontiguousarray(feat[r:r + 1, :A.fbank_frames(n)])), dtype=np.float32)
            if e.reshape(-1).shape[0] != EMBED_DIM:
                raise ValueError(f"the speaker encoder returned {e.size} values for row {r}, expected {EMBED_DIM}")
            rows.append(torch.from_numpy(e.reshape(-1).copy()))
        return torch.stack(rows)
