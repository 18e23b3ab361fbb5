#!/usr/bin/env python3
"""Cost of per-request LoRA adapters at decode (adapters.AdapterBank) on the full-size TransformerLM, bf16, cache L.

For each bank rank R and batch B: us per decoded step (captured graph) of the adapter path -- base weights streamed once,
every row adding its own adapter, B distinct slots -- against the merged path (LoRA folded into the pack) timed in the same
run on the same model.  Also: the down kernel's and the two linears' time per launch (graph of back-to-back launches at the
q|k|v shape), the voice switch (``bank.load`` + first step, against ``load_lora_weights`` + repack + recapture + first step)
and the device bytes per resident voice.

usage: python tools/bench_adapters.py [--dtype bf16] [--batches 1,4,16] [--ranks 16,64] [--len 300] [--steps 100] [--out FILE]
       rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- python tools/bench_adapters.py --steps-only \
           --ranks 16 --batches 1      # per-kernel times inside the step (tools/kernel_avg.py DIR)
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cosyvoice_lora_finetune_framework_amd import decode as D  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.adapters import AdapterBank  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.config import JOINT_TRAINING_CONFIG  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.llm_model import build_llm_model  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.lora import apply_lora_to_model, load_lora_weights  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.modules import Numerics  # noqa: E402


def random_adapter(lm, r, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for n, p in lm.named_parameters():
        if "lora_A" in n:
            sd[n] = torch.randn(r, p.shape[1], generator=g) / p.shape[1] ** 0.5
        elif "lora_B" in n:
            sd[n] = torch.randn(p.shape[0], r, generator=g) * 0.01
    return sd


def time_steps(sess, steps):
    sess.advance(True)                            # (capture on first use + one warm step)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        sess.advance(True)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def graph_us(fn, n=200, reps=5):
    """us per call of fn from a captured graph of n back-to-back calls on one stream (so: kernel + boundary)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (n * reps)


def launch_times(dev, wdt, R, M):
    """per-launch us at the q|k|v shape (K 1024, N 3072, G 3) and at w_2's (K 4096, N 1024)."""
    out = {}
    for tag, K, N, G in (("qkv", 1024, 3072, 3), ("w_2", 4096, 1024, 1)):
        x = torch.randn(M, K, device=dev)
        W = torch.randn(N, K, device=dev).to(wdt)
        A = torch.randn(16, G, R, K, device=dev).to(wdt)
        Bst = torch.randn(16, N, R, device=dev).to(wdt)
        sc = torch.ones(16, device=dev)
        slot = torch.arange(M, dtype=torch.int32, device=dev)
        z = torch.zeros(M, G * R, device=dev)
        y = torch.zeros(M, N, device=dev)
        out[tag] = dict(
            down_us=round(graph_us(lambda: D.decode_lora_down(x, A, slot, out=z)), 3),
            linear_us=round(graph_us(lambda: D.decode_linear(x, W, out=y)), 3),
            linear_lora_us=round(graph_us(lambda: D.decode_linear_lora(x, W, Bst, sc, slot, z, G, out=y)), 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--len", type=int, default=300)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps-only", action="store_true", help="skip the per-launch micro-benchmarks and the voice switch "
                    "(for a kernel trace of the decode steps alone)")
    a = ap.parse_args()
    torch.manual_seed(0)
    wdt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    num = Numerics(dtype=wdt)
    cfg = JOINT_TRAINING_CONFIG["llm_lora"]
    res = dict(dtype=a.dtype, L=a.len, steps=a.steps, ranks={})
    tmp = tempfile.mkdtemp()
    for R in [int(v) for v in a.ranks.split(",")]:
        lm = build_llm_model(None, "cpu", numerics=num)
        apply_lora_to_model(lm, r=R, lora_alpha=2 * R, lora_dropout=0.0, target_modules=cfg["target_modules"])
        lm = lm.to("cuda").eval()
        dev = lm.llm_decoder.weight.device
        voices = [random_adapter(lm, R, 100 + i) for i in range(17)]
        for i in (0, 16):
            torch.save(voices[i], os.path.join(tmp, f"v{i}.pt"))
        load_lora_weights(lm, os.path.join(tmp, "v0.pt"))             # the merged path decodes voice 0
        bank = AdapterBank(llm=lm, capacity=16, rank=R)
        for i in range(16):
            bank.load(f"v{i}", voices[i])
        rec = dict(rows=[], launches={})
        n = 3 * a.steps + 8
        for B in [int(v) for v in a.batches.split(",")]:
            rows = [torch.randn(a.len, lm.llm_input_size, device=dev) for _ in range(B)]
            with torch.no_grad():
                merged = lm.decode_session(B, a.len + n)
                merged.start(rows, [n] * B, [n] * B, list(range(B)), D.SamplerCfg("ras"))
                t_m = time_steps(merged, a.steps)
                sess = lm.decode_session(B, a.len + n, bank=bank)
                sess.start(rows, [n] * B, [n] * B, list(range(B)), D.SamplerCfg("ras"),
                           slots=[bank.slot(f"v{i}") for i in range(B)])
                t_a = time_steps(sess, a.steps)
            r = dict(R=R, B=B, distinct_slots=B, us_per_step_merged=round(t_m, 2), us_per_step_adapters=round(t_a, 2),
                     delta_us=round(t_a - t_m, 2), ratio=round(t_a / t_m, 3))
            print(json.dumps(r), flush=True)
            rec["rows"].append(r)
            if not a.steps_only:
                rec["launches"][f"M{B}"] = launch_times(dev, wdt, R, B)
                print(json.dumps(rec["launches"][f"M{B}"]), flush=True)
        if a.steps_only:
            res["ranks"][str(R)] = rec
            continue
        # voice switch at B = 1: a 17th voice, never seen by either path
        B = 1
        rows = [torch.randn(a.len, lm.llm_input_size, device=dev)]
        with torch.no_grad():
            sess = lm.decode_session(B, a.len + n, bank=bank)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bank.load("v16", os.path.join(tmp, "v16.pt"))                 # evicts the least recently used voice
            bank.activate("v16")
            sess.start(rows, [n], [n], [0], D.SamplerCfg("ras"), slots=[bank.slot("v16")])
            sess.advance(True)
            torch.cuda.synchronize()
            t_bank = time.perf_counter() - t0
            t0 = time.perf_counter()
            load_lora_weights(lm, os.path.join(tmp, "v16.pt"))
            merged = lm.decode_session(B, a.len + n)                     # repack (every parameter's version is checked)
            merged.start(rows, [n], [n], [0], D.SamplerCfg("ras"))
            merged.advance(True)                                         # recapture
            torch.cuda.synchronize()
            t_merged = time.perf_counter() - t0
        rec["voice_switch_ms"] = dict(bank_load_plus_first_step=round(t_bank * 1e3, 2),
                                      load_lora_weights_repack_recapture_first_step=round(t_merged * 1e3, 2),
                                      note="both include the prefill of %d rows" % a.len)
        rec["bytes_per_voice"] = bank.nbytes_per_voice("v16")
        rec["merged_pack_bytes"] = sum(t.numel() * t.element_size() for L in merged.stack.layers for k, t in L.items()
                                       if k in ("Wqkv", "Wo", "W1", "W2"))
        print(json.dumps({k: rec[k] for k in ("voice_switch_ms", "bytes_per_voice", "merged_pack_bytes")}), flush=True)
        res["ranks"][str(R)] = rec
        del lm, bank, sess, merged
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
