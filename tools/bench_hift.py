#!/usr/bin/env python3
"""Time of one utterance through the HiFT vocoder (hift.HiFTGenerator.inference, csrc/hift.hip), B = 1.

For T = 100 / 500 / 1000 mel frames and both weight dtypes: `--warmup` runs, then device events around `--runs` runs
(>= 20) of the whole inference (f0 predictor, source, decode).  Prints the algorithmic FLOP count derived from the
module's shapes (hift.conv_flops: 2 FLOPs per multiply-add of every convolution) and the achieved TFLOP/s.  As a
yardstick the same math runs through torch's own GPU ops (F.conv1d, F.conv_transpose1d, torch.stft / istft) on the
folded fp32 weights in the same process (`torch_vocoder` below; it is not a product path).  One JSON line per
configuration; --out writes the list.

usage: python tools/bench_hift.py [--frames 100,500,1000] [--runs 20] [--warmup 3] [--out profiles/r6_hift_bench.json]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cosyvoice_lora_finetune_framework_amd import hift as Hm  # noqa: E402


def torch_vocoder(m, wdtype=torch.float32):
    """-> fn(mel, phase, noise) -> wav: HiFTGenerator.inference restated with torch's GPU ops on the folded weights."""
    fw = lambda c: (Hm._folded(c).to(wdtype), c.bias.detach().to(wdtype))           # noqa: E731
    f0c = [fw(m.f0_predictor.condnet[2 * i]) for i in range(5)]
    cls = m.f0_predictor.classifier
    pre, post, ups = fw(m.conv_pre), fw(m.conv_post), [fw(u) for u in m.ups]
    rbs = lambda blocks: [[(fw(c1), fw(c2), a1.alpha.detach()[None, :, None], a2.alpha.detach()[None, :, None], d)  # noqa: E731
                           for c1, c2, a1, a2, d in zip(rb.convs1, rb.convs2, rb.activations1, rb.activations2, rb.dilations)]
                          for rb in blocks]
    main_rb, src_rb = rbs(m.resblocks), rbs(m.source_resblocks)
    win = torch.hann_window(16, periodic=True, device=cls.weight.device)
    snake = lambda x, a: x + (1.0 / (a + 1e-9)) * torch.sin(x * a) ** 2               # noqa: E731

    def conv(x, wb, d=1):
        w, b = wb
        return F.conv1d(x.to(wdtype), w, b, dilation=d, padding=(w.shape[2] - 1) // 2 * d).float()

    def resblock(x, rb):
        for c1, c2, a1, a2, d in rb:
            x = conv(snake(conv(snake(x, a1), c1, d), a2), c2) + x
        return x

    def run(mel, phase, noise):
        h = mel
        for wb in f0c:
            h = F.elu(conv(h, wb))
        f0 = F.linear(h.transpose(1, 2), cls.weight, cls.bias).squeeze(-1).abs()        # [B, T]
        f0u = f0.repeat_interleave(256, dim=1)[:, None]
        harm = torch.arange(1, 10, device=mel.device, dtype=torch.float32)[None, :, None]
        theta = 2 * math.pi * (torch.cumsum((f0u * harm / 22050).double(), -1).float() % 1)
        uv = (f0u > 10).float()
        sines = 0.1 * torch.sin(theta + phase) * uv + (uv * 0.003 + (1 - uv) * 0.1 / 3) * noise
        s = torch.tanh(F.linear(sines.transpose(1, 2), m.m_source.l_linear.weight, m.m_source.l_linear.bias))[..., 0]
        spec = torch.stft(s, 16, 4, 16, window=win, return_complex=True)
        s_stft = torch.cat([spec.real, spec.imag], 1)
        x = conv(mel, pre)
        for i in range(2):
            w, b = ups[i]
            x = F.conv_transpose1d(F.leaky_relu(x, 0.1).to(wdtype), w, b, stride=8, padding=4).float()
            if i == 1:
                x = F.pad(x, (1, 0), mode="reflect")
            x = x + resblock(m.source_downs[i](s_stft), src_rb[i])
            x = sum(resblock(x, main_rb[3 * i + j]) for j in range(3)) / 3
        x = conv(F.leaky_relu(x), post)
        mag, ph = torch.exp(x[:, :9]).clamp(max=1e2), torch.sin(x[:, 9:])
        return torch.istft(torch.complex(mag * torch.cos(ph), mag * torch.sin(ph)), 16, 4, 16, window=win).clamp(-0.99, 0.99)
    return run


def timed(fn, runs: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(runs):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="100,500,1000")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch yardstick (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 20 or a.no_torch, "--runs >= 20"
    torch.manual_seed(0)
    dev = torch.device("cuda")
    m = Hm.HiFTGenerator().to(dev).eval()
    res = []
    with torch.no_grad():
        for T in [int(v) for v in a.frames.split(",")]:
            mel = torch.randn(1, 80, T, device=dev) * 1.5 - 3.0
            draws = m.make_draws(1, T * 256, 0, dev)
            flops = Hm.conv_flops(m, T)
            for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
                ms = timed(lambda: m.inference(mel, draws=draws, dtype=dt), a.runs, a.warmup)
                r = dict(T=T, dtype=name, ms_per_utterance=round(ms, 3), gflop=round(flops / 1e9, 1),
                         tflops=round(flops / (ms * 1e-3) / 1e12, 2), audio_s=round(T * 256 / 22050, 2))
                if not a.no_torch:
                    ref = torch_vocoder(m, dt)
                    r["torch_ops_ms"] = round(timed(lambda: ref(mel, draws[0], draws[1]), a.runs, a.warmup), 3)
                    if dt == torch.float32:         # the yardstick computes the same thing
                        d = (ref(mel, draws[0], draws[1]) - m.inference(mel, draws=draws, dtype=dt)[0]).abs().max()
                        r["torch_ops_max_abs_diff"] = float(d)
                print(json.dumps(r), flush=True)
                res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
