"""Wavs + precomputed tokens -> the parquet shards ``dataset.FlowFinetuneDataset`` reads: the mel leg and the writer of
the reference's ``prepare_joint_data.py``.

    python -m cosyvoice_lora_finetune_framework_amd.prepare_joint_data --manifest m.jsonl --output-dir D \\
        [--samples-per-file 100] [--batch 16] [--speech-tokenizer speech_tokenizer_v1.onnx] [--campplus campplus.onnx]

Each manifest line is a JSON object with ``utt``, ``wav`` (16-bit PCM at 22 050 Hz; a relative path is taken from the
manifest's directory), ``text``, ``text_token``, ``speech_token`` (id lists) and ``utt_embedding`` (192 floats).  The
reference computes those three with its text tokenizer and two ONNX models (speech tokenizer, speaker encoder), which
this project does not rebuild, so they come precomputed; what is computed here is ``speech_feat``,
the [T, 80] log-mel the Flow is trained on, on the GPU (``audio.MelExtractor``) in length-sorted ragged batches.
Files that are not at 22 050 Hz are resampled to it on the GPU first (``audio.Resampler``), as the reference does with
torchaudio (prepare_joint_data.py:172-174).  ``--resampled-dir`` with ``--resampled-rate`` also writes every kept
utterance resampled to that rate as ``<utt>.wav`` (16-bit PCM): 16 000 Hz is what the reference's speech tokenizer and
speaker encoder take, so their inputs need no other tool.

With ``--speech-tokenizer`` / ``--campplus`` (the reference's two ONNX files; ``onnxruntime`` runs them on the CPU) the
matching manifest key becomes optional: an entry without ``speech_token`` / ``utt_embedding`` gets it computed, per batch,
from the 16 kHz resample of the audio already on the device -- the Whisper log-mel and the Kaldi fbank are formed on the GPU
(``audio.whisper_log_mel`` / ``audio.kaldi_fbank``; ``frontend16k.SpeechFrontend``).  A value the manifest carries wins.
Without the two options nothing changes, the error for a missing key included.

Like the reference (prepare_joint_data.py:252-256) utterances shorter than 0.5 s or longer than 30 s are dropped.
Output: ``data_%06d.parquet`` with the reference's columns -- utt, text, text_token, speech_token, speech_feat
(flattened), speech_feat_shape, utt_embedding, spk_embedding -- and ``data.list`` naming the shards.
"""
from __future__ import annotations

import argparse
import json
import os
import wave
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import audio as A

MIN_SECONDS, MAX_SECONDS = 0.5, 30.0
REQUIRED = ("utt", "wav", "text", "text_token", "speech_token", "utt_embedding")
COLUMNS = ("utt", "text", "text_token", "speech_token", "speech_feat", "speech_feat_shape", "utt_embedding", "spk_embedding")


def read_manifest(path: str, computed: Tuple[str, ...] = ()) -> List[Dict[str, Any]]:
    """JSON lines -> entries with every REQUIRED key; `wav` resolved against the manifest's directory.  Keys named in
    `computed` (speech_token, utt_embedding) may be absent: the caller has a model that fills them."""
    base = os.path.dirname(os.path.abspath(path))
    out = []
    with open(path, "r", encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            e = json.loads(line)
            missing = [k for k in REQUIRED if k not in e and k not in computed]
            if missing:
                raise ValueError(f"{path}:{no}: missing {', '.join(missing)}")
            if not e["text_token"] or ("speech_token" in e and not e["speech_token"]):
                raise ValueError(f"{path}:{no}: {e['utt']}: empty token list")
            e = dict(e)
            if not os.path.isabs(e["wav"]):
                e["wav"] = os.path.join(base, e["wav"])
            out.append(e)
    return out


def keep_duration(n_samples: int, rate: int) -> bool:
    """the reference's duration filter: 0.5 s <= duration <= 30 s."""
    return MIN_SECONDS <= n_samples / rate <= MAX_SECONDS


def wav_info(path: str) -> Tuple[int, int]:
    """(samples per channel, rate) from the file's header."""
    with wave.open(path, "rb") as f:
        return f.getnframes(), f.getframerate()


def filter_entries(entries: List[Dict[str, Any]], verbose: bool = True) -> List[Dict[str, Any]]:
    kept = []
    for e in entries:
        n, rate = wav_info(e["wav"])
        if keep_duration(n, rate):
            kept.append(e)
        elif verbose:
            print(f"  skip {e['utt']}: {n / rate:.1f} s outside [{MIN_SECONDS}, {MAX_SECONDS}]")
    return kept


def _batches(wavs: List[torch.Tensor], rates: List[int], batch: int):
    """(rate, entry indices, lengths, zero-padded [rows, max length] CPU tensor) per batch: one source rate per batch,
    batches formed after sorting by length."""
    for rate in sorted(set(rates)):
        order = sorted((i for i in range(len(wavs)) if rates[i] == rate), key=lambda i: wavs[i].shape[0])
        for i0 in range(0, len(order), batch):
            idx = order[i0:i0 + batch]
            lens = [wavs[i].shape[0] for i in idx]
            pad = torch.zeros(len(idx), max(lens))
            for r, i in enumerate(idx):
                pad[r, :lens[r]] = wavs[i]
            yield rate, idx, lens, pad


def extract_feats(entries: List[Dict[str, Any]], device, batch: int = 16, resampled_dir: Optional[str] = None,
                  resampled_rate: Optional[int] = None, frontend=None) -> List[torch.Tensor]:
    """speech_feat [T, 80] (CPU fp32) per entry, in the entries' order.  Files at another rate than 22 050 Hz are
    resampled to it on the GPU, batched per source rate; with `resampled_dir` every entry is also written there as
    <utt>.wav at `resampled_rate`.  With `frontend` (frontend16k.SpeechFrontend) the entries that lack speech_token /
    utt_embedding get them, in place, from the batch's 16 kHz resample and the frontend's models."""
    ext = A.extractor(device)
    wavs, rates = [], []
    for e in entries:
        w, rate = A.load_wav(e["wav"])
        wavs.append(w)
        rates.append(int(rate))
    feats: List[Any] = [None] * len(wavs)
    for rate, idx, lens, pad in _batches(wavs, rates, batch):
        x = pad.to(device)
        y, ylens = A.resample(x, rate, A.SAMPLE_RATE, lens)
        mel = ext(y, ylens, channel_last=True).cpu()
        for r, i in enumerate(idx):
            feats[i] = mel[r, :A.n_frames(ylens[r])].contiguous()
        if resampled_dir is not None:
            from .inference_joint import write_wav
            z, zlens = A.resample(x, rate, resampled_rate, lens)
            z = z.cpu()
            for r, i in enumerate(idx):
                write_wav(os.path.join(resampled_dir, f"{entries[i]['utt']}.wav"), z[r, :zlens[r]], int(resampled_rate))
        if frontend is not None:
            _fill_from_models(entries, idx, frontend, x, rate, lens)
    return feats


def _fill_from_models(entries, idx, frontend, x: torch.Tensor, rate: int, lens: List[int]) -> None:
    """speech_token / utt_embedding of the batch's entries that lack them: one feature call per model over those rows."""
    for key, have in (("speech_token", frontend.speech_tokenizer), ("utt_embedding", frontend.speaker_encoder)):
        rows = [r for r, i in enumerate(idx) if key not in entries[i]]
        if have is None or not rows:
            continue
        sub = x if len(rows) == len(idx) else x[rows, :max(lens[r] for r in rows)].contiguous()
        z, zlens = A.resample(sub, rate, A.FRONTEND_RATE, [lens[r] for r in rows])
        if key == "speech_token":
            for r, ids in zip(rows, frontend.tokens(z, zlens)):
                if not ids:
                    raise ValueError(f"{entries[idx[r]]['utt']}: the speech tokenizer returned no tokens")
                entries[idx[r]][key] = ids
        else:
            for r, emb in zip(rows, frontend.embeddings(z, zlens)):
                entries[idx[r]][key] = emb.tolist()


def make_row(e: Dict[str, Any], feat: torch.Tensor) -> Dict[str, Any]:
    emb = [float(v) for v in e["utt_embedding"]]
    return {"utt": e["utt"], "text": e["text"], "text_token": [int(v) for v in e["text_token"]],
            "speech_token": [int(v) for v in e["speech_token"]], "speech_feat": feat.reshape(-1).tolist(),
            "speech_feat_shape": [int(feat.shape[0]), int(feat.shape[1])], "utt_embedding": emb, "spk_embedding": emb}


def write_shard(rows: List[Dict[str, Any]], output_dir: str, index: int) -> str:
    import pyarrow as pa
    import pyarrow.parquet as pq
    path = os.path.join(output_dir, f"data_{index:06d}.parquet")
    pq.write_table(pa.Table.from_pydict({c: [r[c] for r in rows] for c in COLUMNS}), path)
    return path


def prepare(manifest: str, output_dir: str, samples_per_file: int = 100, batch: int = 16, device="cuda",
            verbose: bool = True, resampled_dir: Optional[str] = None, resampled_rate: Optional[int] = None,
            speech_tokenizer=None, speaker_encoder=None) -> List[str]:
    """-> the shard paths written (also listed in output_dir/data.list).  `speech_tokenizer` / `speaker_encoder`: the
    callables of frontend16k.SpeechFrontend; with one given, entries may lack speech_token / utt_embedding."""
    if (resampled_dir is None) != (resampled_rate is None):
        raise ValueError("--resampled-dir and --resampled-rate go together")
    os.makedirs(output_dir, exist_ok=True)
    if resampled_dir is not None:
        os.makedirs(resampled_dir, exist_ok=True)
    frontend = None
    if speech_tokenizer is not None or speaker_encoder is not None:
        from .frontend16k import SpeechFrontend
        frontend = SpeechFrontend(device, speech_tokenizer, speaker_encoder)
    computed = tuple(k for k, m in (("speech_token", speech_tokenizer), ("utt_embedding", speaker_encoder)) if m is not None)
    entries = filter_entries(read_manifest(manifest, computed), verbose)
    if not entries:
        raise RuntimeError(f"{manifest}: no utterance left after the duration filter")
    shards = []
    for i0 in range(0, len(entries), samples_per_file):
        part = entries[i0:i0 + samples_per_file]
        feats = extract_feats(part, device, batch, resampled_dir, resampled_rate, frontend)
        rows = [make_row(e, f) for e, f in zip(part, feats)]
        shards.append(write_shard(rows, output_dir, len(shards)))
        if verbose:
            print(f"  wrote {shards[-1]} ({len(rows)} utterances)")
    with open(os.path.join(output_dir, "data.list"), "w") as f:
        for p in shards:
            f.write(p + "\n")
    return shards


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--manifest", required=True, help="JSON lines: utt, wav, text, text_token, speech_token, utt_embedding")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--samples-per-file", type=int, default=100)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--resampled-dir", default=None, help="also write every kept utterance here as <utt>.wav at --resampled-rate")
    ap.add_argument("--resampled-rate", type=int, default=None, help="rate of the files in --resampled-dir, e.g. 16000")
    ap.add_argument("--speech-tokenizer", default=None, help="the speech tokenizer's .onnx: speech_token becomes optional")
    ap.add_argument("--campplus", default=None, help="the speaker encoder's .onnx: utt_embedding becomes optional")
    a = ap.parse_args(argv)
    models = {}
    if a.speech_tokenizer or a.campplus:
        from .frontend16k import SpeechFrontend
        fe = SpeechFrontend.from_onnx(a.speech_tokenizer, a.campplus)
        models = dict(speech_tokenizer=fe.speech_tokenizer, speaker_encoder=fe.speaker_encoder)
    shards = prepare(a.manifest, a.output_dir, a.samples_per_file, a.batch, resampled_dir=a.resampled_dir,
                     resampled_rate=a.resampled_rate, **models)
    print(f"{len(shards)} shard(s) -> {os.path.join(a.output_dir, 'data.list')}")


if __name__ == "__main__":
    main()
