#!/usr/bin/env python3
"""Decode-step timing of the full-size TransformerLM (14 layers, d 1024, V 4097) on the decode kernels.

For each batch B and cache length L: prefill B rows of L random lm_input rows, then time `--steps` decode steps
(embedding gather -> 14 layers -> decoder -> sampler) replayed from the captured hipGraph and launched eagerly, with
device events around the whole run.  Reports us per decoded step and the effective weight-stream rate (weight bytes
of one step / step time).  Writes one JSON line per configuration (and a summary to --out).

usage: python tools/bench_decode.py [--dtype bf16] [--batches 1,4,16] [--lens 300,1000] [--steps 100] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cosyvoice_lora_finetune_framework_amd.decode import SamplerCfg  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.llm_model import build_llm_model  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.modules import Numerics  # noqa: E402


def weight_bytes(sess) -> int:
    n = sum(t.numel() * t.element_size() for L in sess.stack.layers for k, t in L.items()
            if k in ("Wqkv", "Wo", "W1", "W2"))
    return n + sess.stack.W_emb.numel() * sess.stack.W_emb.element_size() + sess.W_dec.numel() * sess.W_dec.element_size()


def time_steps(sess, steps: int, use_graph: bool) -> float:
    sess.advance(use_graph)                       # (capture on first use + one warm step)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        sess.advance(use_graph)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--lens", default="300,1000")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    num = Numerics(dtype=torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    lm = build_llm_model(None, "cuda", numerics=num).eval()
    dev = lm.llm_decoder.weight.device
    res = []
    for L in [int(v) for v in a.lens.split(",")]:
        for B in [int(v) for v in a.batches.split(",")]:
            n = 3 * a.steps + 8
            sess = lm.decode_session(B, L + n)
            rows = [torch.randn(L, lm.llm_input_size, device=dev) for _ in range(B)]
            with torch.no_grad():
                sess.start(rows, [n] * B, [n] * B, list(range(B)), SamplerCfg("ras"))
                g = time_steps(sess, a.steps, True)
                e = time_steps(sess, a.steps, False)
            wb = weight_bytes(sess)
            r = dict(dtype=a.dtype, B=B, L=L, us_per_step_graph=round(g, 2), us_per_step_eager=round(e, 2),
                     eager_over_graph=round(e / g, 2), weight_MB=round(wb / 1e6, 1),
                     weight_GBps_graph=round(wb / (g * 1e-6) / 1e9, 1))
            print(json.dumps(r), flush=True)
            res.append(r)
            del sess
            lm.__dict__.get("_cvft_sessions", {}).clear()
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
