#!/usr/bin/env python3
"""ms per call of the resampler (audio.Resampler -> cvft_resample) for 1 s, 10 s and 30 s of audio at B = 1 and B = 16,
for 16 k -> 22.05 k, 48 k -> 22.05 k and 22.05 k -> 16 k, the achieved GB/s of (input + output bytes), and the same math
through torch's own GPU ops on the same GPU in the same process: the dense strided F.conv1d formulation (zero padding,
one n-channel convolution of stride o over the dense [n, 2 width + o] table, channels interleaved, trimmed).  Device
events around 20 calls after 3 warm-ups; prints one JSON object and writes it to --out (profiles/r9_resample_bench.json).

usage: python tools/bench_resample.py [--out profiles/r9_resample_bench.json] [--runs 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cosyvoice_lora_finetune_framework_amd import audio as A  # noqa: E402

PAIRS = [(16000, 22050), (48000, 22050), (22050, 16000)]


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r9_resample_bench.json"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    g = torch.Generator().manual_seed(0)
    for orig, new in PAIRS:
        rs = A.Resampler(orig, new, dev)
        K, width, o, n = A.sinc_kernel(orig, new)
        dense = torch.from_numpy(K).to(dev).unsqueeze(1)                       # [n, 1, 2 width + o]

        def torch_path(x, M):
            y = F.conv1d(F.pad(x, (width, width + o)).unsqueeze(1), dense, stride=o)   # [B, n, J]
            return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :M]

        for seconds in (1, 10, 30):
            for B in (1, 16):
                L = seconds * orig
                M = A.resampled_length(L, orig, new)
                x = (torch.rand(B, L, generator=g) * 0.6 - 0.3).to(dev)
                diff = float((rs(x)[0] - torch_path(x, M)).abs().max())
                k = timed(lambda: rs(x), a.runs, a.warmup)
                t = timed(lambda: torch_path(x, M), a.runs, a.warmup)
                nbytes = 4.0 * B * (L + M)
                rows.append(dict(orig=orig, new=new, seconds=seconds, B=B, samples_in=B * L, samples_out=B * M, span=rs.span,
                                 cvft_resample=k, torch_conv1d_dense=t, max_abs_diff=diff,
                                 gbps=nbytes / (k["median_ms"] * 1e-3) / 1e9,
                                 torch_gbps=nbytes / (t["median_ms"] * 1e-3) / 1e9))
    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, warmup=a.warmup, tile=A.RESAMPLE_TILE, rows=rows)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
