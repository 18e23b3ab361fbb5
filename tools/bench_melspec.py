#!/usr/bin/env python3
"""ms per call of the mel front-end (audio.MelExtractor -> cvft_melspec) for 1 s, 10 s and 30 s of audio at B = 1 and
B = 16, next to the same math through torch.stft + matmul on the same GPU in the same process.  Device events around
20 calls after 3 warm-ups; prints one JSON object and writes it to --out (profiles/r7_melspec_bench.json).

usage: python tools/bench_melspec.py [--out profiles/r7_melspec_bench.json] [--runs 20] [--warmup 3]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r7_melspec_bench.json"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ext = A.MelExtractor(dev)
    basis = torch.from_numpy(ext.basis).to(dev)
    window = torch.hann_window(A.WIN, device=dev)

    def torch_path(x):
        y = torch.nn.functional.pad(x.unsqueeze(1), (A.REFLECT, A.REFLECT), mode="reflect").squeeze(1)
        spec = torch.view_as_real(torch.stft(y, A.N_FFT, hop_length=A.HOP, win_length=A.WIN, window=window, center=False,
                                             normalized=False, onesided=True, return_complex=True))
        return torch.log(torch.clamp(torch.matmul(basis, torch.sqrt(spec.pow(2).sum(-1) + 1e-9)), min=1e-5))

    rows = []
    g = torch.Generator().manual_seed(0)
    for seconds in (1, 10, 30):
        for B in (1, 16):
            L = seconds * A.SAMPLE_RATE
            x = (torch.rand(B, L, generator=g) * 0.6 - 0.3).to(dev)
            diff = float((ext(x) - torch_path(x)).abs().max())
            k = timed(lambda: ext(x), a.runs, a.warmup)
            t = timed(lambda: torch_path(x), a.runs, a.warmup)
            frames = B * (L // A.HOP)
            flop = frames * (2.0 * 2 * 16 * ext.nchunks * A.N_FFT + 2.0 * 80 * 16 * ext.nchunks)
            rows.append(dict(seconds=seconds, B=B, frames=frames, cvft_melspec=k, torch_stft_matmul=t,
                             max_abs_diff=diff, gemm_tflops=flop / (k["median_ms"] * 1e-3) / 1e12))
    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, warmup=a.warmup, rows=rows)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
