"""Plan equals launch: for one launch of every kernel family cvft_gemm chooses between, cvft_gemm_plan (asked about the very
arguments of the launch, just before it) names the kernel that cvft_gemm_last_kernel() reports afterwards, the planned row
ranges tile [0, M), and the result matches an fp64 product at the tolerance of tests/test_ops_gpu.py."""
import math

import pytest
import torch

import dispatch_fixture as DF
from helpers import keep_scale_host

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}      # tests/test_ops_gpu.py
BF, F32 = torch.bfloat16, torch.float32

#        name            dtype M     N     K    kind     R   kernel the case is about
CASES = [("skinny",      BF, 300,   32,  256, "plain",  0, "skinny_kernel<bf16,r32>"),
         ("glds_64x64",  BF, 300,  512,  256, "bias",   0, "gemm_glds_kernel<bf16,64,64,2,2,"),
         ("glds_128x64", BF, 4100, 1004, 256, "bias",   0, "gemm_glds_kernel<bf16,128,64,4,2,"),
         ("glds_128x128", BF, 4200, 2052, 512, "bias",  0, "gemm_glds_kernel<bf16,128,128,4,2,"),
         ("glds_96x256", BF, 4000, 1000, 512, "bias",   0, "gemm_glds_kernel<bf16,96,256,3,4,"),
         ("fused_r16",   BF, 300,  512,  256, "fused", 16, ",fusedU16"),
         ("fused_r48",   BF, 300,  512,  256, "fused", 48, ",fusedU48"),
         ("xdrop",       BF, 300,  512,  256, "xdrop", 16, ",xdrop"),
         ("staged_k224", BF, 300,  512,  224, "bias",   0, "gemm_kernel<bf16,64,64,2,2>"),
         ("generic_k100", BF, 300, 512,  100, "bias",   0, "gemm_kernel<bf16,64,64,2,2>"),
         ("fp32",        F32, 300, 512,  128, "bias",   0, "gemm_kernel<f32,64,64,2,2>"),
         ("p256",        BF, 2048, 6144, 512, "bias",   0, "gemm_p256_kernel<bf16,256,256,2,4,ring10>"),
         ("p256_rowsplit", BF, 2304, 8192, 512, "bias", 0, "gemm_p256_kernel<bf16,256,256,2,4,ring10>")]


def _rel(a, b):
    return float((a.double() - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("name,dtype,M,N,K,kind,R,kernel", CASES, ids=[c[0] for c in CASES])
def test_plan_names_the_launch_and_the_launch_is_right(name, dtype, M, N, K, kind, R, kernel):
    from cosyvoice_lora_finetune_framework_amd.hipops import functional as HF
    lib = HF.lib()
    g = torch.Generator(device=DEV).manual_seed(7)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device=DEV) * scale).to(dtype)      # noqa: E731
    x, w = rn(M, K), rn(N, K, scale=1 / math.sqrt(K))
    ref = x.double() @ w.double().t()
    kw = {}
    if kind == "bias":
        kw["bias"] = torch.randn(N, generator=g, device=DEV)
        ref += kw["bias"].double()
    elif kind == "fused":
        la, bl = rn(R, K, scale=1 / math.sqrt(K)), rn(N, R, scale=0.1)
        kw.update(La=la, lora_scale=2.0, Uout=torch.empty(M, R, device=DEV, dtype=dtype), Bl=bl)
        u = (2.0 * (x.double() @ la.double().t())).to(dtype).double()        # the kernel feeds the rounded U to the extension step
        ref += u @ bl.double().t()
    elif kind == "xdrop":
        u, bl, p, site = rn(M, R), rn(N, R, scale=0.1), 0.15, 11
        HF.dropout_begin_step()
        keep = keep_scale_host(int(HF._DROPOUT["seed"].item()), site, M * N, p).view(M, N).to(DEV)
        kw.update(U=u, Bl=bl, xdrop=(p, [site]))
        ref += keep * (u.double() @ bl.double().t())
    with DF.planned(lib) as plans:
        y = HF.gemm(x, w, **kw)
    launched = lib.cvft_gemm_last_kernel().decode()
    torch.cuda.synchronize()
    assert len(plans) == 1 and plans[0][0] == 0, plans
    lines = DF.plan_lines(plans[0][1])
    assert lines[-1][0] == launched and kernel in launched, (lines, launched)
    assert len(lines) == (2 if name == "p256_rowsplit" else 1), lines
    rows = sorted((r0, n) for _, r0, n in lines)
    assert rows[0][0] == 0 and sum(n for _, n in rows) == M and all(a[0] + a[1] == b[0] for a, b in zip(rows, rows[1:])), lines
    if name == "p256_rowsplit":
        assert lines[0][0].startswith("gemm_glds_kernel<bf16,") and lines[0][1:] == (2048, 256) and lines[1][1:] == (0, 2048), lines
    assert _rel(y, ref) < TOL[dtype]
    if kind == "fused":
        assert _rel(kw["Uout"], 2.0 * (x.double() @ la.double().t())) < TOL[dtype]
