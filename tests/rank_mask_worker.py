"""Child process of tests/test_lora_rank_masked_gpu.py: one LinearFn and one stacked q|k|v forward + backward in train mode under
the CVFT_RANK_MASK setting of its environment (read at import of hipops.functional, hence a fresh process per setting).
usage: rank_mask_worker.py OUT.pt"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cosyvoice_lora_finetune_framework_amd.hipops import functional as HF  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.lora import LoRALinear  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.modules import hip_linear, hip_qkv  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.optim import FlatAdamW  # noqa: E402

DEV = "cuda"
K, N, M = 256, 512, 1000


def step(fn, opt, params):
    """-> (gradients, dropped copies alive between forward and backward, peak allocated bytes above the starting level)"""
    opt.zero_grad()
    HF.dropout_begin_step()
    HF._DROPOUT["seed"].fill_(4242)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with HF.LoraGradSink():
        outs, grads = fn()
        held = len(HF._DROPPED)
        torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    return [p.grad.clone() for p in params], held, torch.cuda.max_memory_allocated() - base


def main(out_path):
    torch.manual_seed(11)
    res = {"rank_mask": HF.RANK_MASK}
    x = (torch.randn(M, K, device=DEV) * 0.5).to(torch.bfloat16)
    # one LoRA linear under lora_dropout (LinearFn)
    lin = LoRALinear(torch.nn.Linear(K, N), r=16, lora_alpha=32, lora_dropout=0.05).to(DEV).train()
    torch.nn.init.normal_(lin.lora_B, std=0.05)
    params = [lin.lora_A, lin.lora_B]
    opt = FlatAdamW(params, lr=1e-3)
    g = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    xi = x.clone().requires_grad_(True)

    def run_linear():
        y = hip_linear(lin, xi)
        assert type(y.grad_fn).__name__.startswith("LinearFn")
        return [y], [g]
    for _ in range(2):                       # (second pass: slab workspaces exist, the peak is the step's own)
        xi.grad = None
        grads, held, peak = step(run_linear, opt, params)
    res["linear"] = {"grads": [t.cpu() for t in grads], "dx": xi.grad.cpu(), "held": held, "peak": peak}
    # stacked q|k|v under lora_dropout (LinearQKVStackedFn), in line and postponed to the sink's batch launches
    mods = [LoRALinear(torch.nn.Linear(K, N), r=16, lora_alpha=32, lora_dropout=0.15).to(DEV).train() for _ in range(3)]
    for m in mods:
        torch.nn.init.normal_(m.lora_B, std=0.05)
    qparams = [p for m in mods for p in (m.lora_A, m.lora_B)]
    qopt = FlatAdamW(qparams, lr=1e-3)
    g3 = torch.randn(M, 3 * N, device=DEV).to(torch.bfloat16)
    xq = x.clone().requires_grad_(True)

    def run_qkv():
        q_, k_, v_ = hip_qkv(mods[0], mods[1], mods[2], xq)
        assert "Stacked" in type(q_.grad_fn).__name__
        return [q_, k_, v_], [g3[:, :N], g3[:, N:2 * N], g3[:, 2 * N:]]
    for defer in (False, True):
        HF.STACKED_DROP_DEFER = defer
        for _ in range(2):
            xq.grad = None
            grads, held, peak = step(run_qkv, qopt, qparams)
        res["qkv_defer%d" % defer] = {"grads": [t.cpu() for t in grads], "dx": xq.grad.cpu(), "held": held, "peak": peak}
    torch.save(res, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
