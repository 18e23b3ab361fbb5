#!/usr/bin/env python3
"""ms per call of the two 16 kHz front-ends (audio.whisper_log_mel / audio.kaldi_fbank -> cvft_feat16k + its finishing
launch) for 1 s, 10 s and 30 s of audio at B = 1 and B = 16, next to the same math through torch.stft + matmul on the same
GPU in the same process.  Device events around 20 calls after 3 warm-ups, medians; prints one JSON object and writes it to
--out (profiles/r11_feat16k_bench.json).

usage: python tools/bench_feat16k.py [--out profiles/r11_feat16k_bench.json] [--runs 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from cosyvoice_lora_finetune_framework_amd import audio as A  # noqa: E402


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r11_feat16k_bench.json"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    wh, fb = A.whisper_extractor(dev), A.fbank_extractor(dev)
    wbank, kbank = torch.from_numpy(wh.basis).to(dev), torch.from_numpy(fb.basis).to(dev)
    hann = torch.hann_window(A.FRONT_FRAME, device=dev)
    n = torch.arange(A.FRONT_FRAME, device=dev, dtype=torch.float64)
    povey = ((0.5 - 0.5 * torch.cos(2 * torch.pi * n / (A.FRONT_FRAME - 1))) ** 0.85).float()

    def torch_whisper(x):
        spec = torch.stft(x, A.FRONT_FRAME, A.FRONT_HOP, window=hann, return_complex=True)     # center, reflect
        mel = torch.matmul(wbank, spec[..., :-1].abs() ** 2)
        v = torch.clamp(mel, min=1e-10).log10()
        v = torch.maximum(v, v.amax(dim=(1, 2), keepdim=True) - 8.0)
        return (v + 4.0) / 4.0

    def torch_fbank(x):
        fr = x.unfold(1, A.FRONT_FRAME, A.FRONT_HOP)
        fr = fr - fr.mean(dim=2, keepdim=True)
        fr = fr - A.FBANK_PREEMPH * torch.cat([fr[..., :1], fr[..., :-1]], dim=2)
        spec = torch.fft.rfft(fr * povey, A.FBANK_NFFT)
        v = torch.clamp(torch.matmul(spec.abs() ** 2, kbank.t()), min=A.FBANK_EPS).log()
        return v - v.mean(dim=1, keepdim=True)

    rows = []
    g = torch.Generator().manual_seed(0)
    for seconds in (1, 10, 30):
        for B in (1, 16):
            L = seconds * A.FRONTEND_RATE
            x = (torch.rand(B, L, generator=g) * 0.6 - 0.3).to(dev)
            for name, ours, theirs, nchunks, bands, frames in (
                    ("whisper_log_mel", A.whisper_log_mel, torch_whisper, wh.nchunks, 128, A.whisper_frames(L)),
                    ("kaldi_fbank", A.kaldi_fbank, torch_fbank, fb.nchunks, 80, A.fbank_frames(L))):
                diff = float((ours(x) - theirs(x)).abs().max())
                k = timed(lambda: ours(x), a.runs, a.warmup)
                t = timed(lambda: theirs(x), a.runs, a.warmup)
                flop = B * frames * (2.0 * 2 * 16 * nchunks * A.FRONT_FRAME + 2.0 * bands * 16 * nchunks)
                rows.append(dict(feature=name, seconds=seconds, B=B, frames=B * frames, cvft_feat16k=k, torch_stft_matmul=t,
                                 max_abs_diff=diff, gemm_tflops=flop / (k["median_ms"] * 1e-3) / 1e12))
    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, warmup=a.warmup, rows=rows)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
