"""Host side of the ResnetBlock1D fold (no GPU): the packed weights of the pair launches, restated as the tap-GEMM's own index
arithmetic in fp64 and checked against torch.nn.functional.conv1d and its autograd; and what cvft_gemm_plan says about the
two-output / two-operand launches -- which kernel takes them, and that an ineligible request is an error, not a fall-through."""
import torch
import torch.nn.functional as F

from dispatch_fixture import plan_lines, plan_text


def _taps(x, offs):
    """x [B, T, C] -> [x shifted by each tap offset, zero outside [0, T)] (the kernel's irow_j(m))"""
    B, T, C = x.shape
    out = []
    for o in offs:
        y = torch.zeros_like(x)
        lo, hi = max(0, -o), min(T, T - o)
        y[:, lo:hi] = x[:, lo + o:hi + o]
        out.append(y)
    return out


def test_pair_weights_restate_both_convolutions_and_their_input_gradient():
    """Wf [N1 + N2][3 Cin]: rows < N1 walk all three taps, rows >= N1 only the centre slice (the launch never reads the others,
    which the packing leaves zero).  Wb [Cin][3 N1 + N2]: three flipped slices against dh[t - 1], dh[t], dh[t + 1] and a fourth
    against dr[t].  fp64 against F.conv1d on the masked input and against autograd's input gradient; exact up to summation order."""
    from cosyvoice_lora_finetune_framework_amd.hipops.functional import conv_pair_weights
    g = torch.Generator().manual_seed(0)
    B, T, Cin, N = 2, 11, 24, 64
    lens = torch.tensor([11, 6])
    w3 = torch.randn(N, Cin, 3, generator=g, dtype=torch.float64)
    w1 = torch.randn(N, Cin, 1, generator=g, dtype=torch.float64)
    b3, b1 = torch.randn(N, generator=g, dtype=torch.float64), torch.randn(N, generator=g, dtype=torch.float64)
    x = torch.randn(B, T, Cin, generator=g, dtype=torch.float64)
    mask = (torch.arange(T)[None, :] < lens[:, None]).double()[:, :, None]
    Wf, Wb = conv_pair_weights(w3, w1, torch.float64)
    assert Wf.shape == (2 * N, 3 * Cin) and Wb.shape == (Cin, 4 * N)
    assert float(Wf[N:, :Cin].abs().max()) == 0.0 and float(Wf[N:, 2 * Cin:].abs().max()) == 0.0

    xm = (x * mask).requires_grad_(True)
    a = _taps(xm.detach(), (-1, 0, 1))
    h = sum(a[j] @ Wf[:N, j * Cin:(j + 1) * Cin].t() for j in range(3)) + b3
    r = a[1] @ Wf[N:, Cin:2 * Cin].t() + b1
    hr = F.conv1d(xm.transpose(1, 2), w3, b3, padding=1).transpose(1, 2)
    rr = F.conv1d(xm.transpose(1, 2), w1, b1).transpose(1, 2)
    assert float((h - hr.detach()).abs().max()) < 1e-12 and float((r - rr.detach()).abs().max()) < 1e-12
    # rows at or beyond in_len of the shortcut are its bias
    assert torch.equal(rr.detach()[1, 6:], b1.expand(T - 6, N))

    dh = torch.randn(B, T, N, generator=g, dtype=torch.float64)
    dr = torch.randn(B, T, N, generator=g, dtype=torch.float64)
    (hr * dh).sum().backward(retain_graph=True)
    (rr * dr).sum().backward()
    d = _taps(dh, (-1, 0, 1)) + [dr]
    dx = sum(d[j] @ Wb[:, j * N:(j + 1) * N].t() for j in range(4))
    assert float((dx - xm.grad).abs().max()) < 1e-12


def _args(**kw):
    from cosyvoice_lora_finetune_framework_amd.hipops.binding import BF16, GemmArgs
    a = GemmArgs()
    B, T, Cin, N = 2, 37, 320, 256
    a.dtype, a.M, a.N, a.K = BF16, B * T, 2 * N, Cin
    a.Tm = a.Tin = a.Tout = T
    a.in_stride = a.out_stride = 1
    a.ntaps = 3
    for i, o in enumerate((-1, 0, 1)):
        a.tap_off[i] = o
    a.alpha = 1.0
    a.A, a.lda, a.W, a.ldw = 1 << 36, Cin, 2 << 36, 3 * Cin
    a.C, a.ldc, a.C2, a.ldc2, a.N1 = 3 << 36, N, 4 << 36, N, N
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_pair_launches_go_to_the_kernels_that_implement_them_or_fail():
    from cosyvoice_lora_finetune_framework_amd.hipops import binding as cb
    lib = cb.lib()
    rc, text = plan_text(lib, _args())
    assert rc == 0 and plan_lines(text) == [("gemm_kernel<bf16,64,64,2,2>,two_out", 0, 74)], (rc, text, lib.cvft_last_error())
    # 74 rows x 512 columns of 64x64 tiles
    assert " grid=16 " in text
    # the two-operand dgrad: four taps, K = N = 256, the last tap on A2
    d = _args(N=320, K=256, ntaps=4, lda=256, ldw=4 * 256, ldc=320, C2=None, N1=0, A2=5 << 36, lda2=256)
    rc, text = plan_text(lib, d)
    assert rc == 0 and plan_lines(text)[0][0] == "gemm_kernel<bf16,64,64,2,2>,two_in", (rc, text, lib.cvft_last_error())
    # nothing falls through: every ineligible request is an error
    for bad in (dict(N1=200, N=456), dict(dtype=cb.F32), dict(act=5), dict(residual=6 << 36, ldr=256), dict(A=(1 << 36) + 2),
                dict(K=324, lda=324, ldw=3 * 324), dict(A2=5 << 36, lda2=320), dict(Bl=7 << 36, ldbl=16, R=16), dict(Uout=7 << 36)):
        rc, text = plan_text(lib, _args(**bad))
        assert rc != 0 and text == "", (bad, rc, text)
        assert b"cvft_gemm" in lib.cvft_last_error()
    rc, _ = plan_text(lib, _args(N=320, K=256, ntaps=4, lda=256, ldw=4 * 256, ldc=320, C2=None, N1=0, A2=5 << 36, lda2=256, Bl=7 << 36, ldbl=16, R=16))
    assert rc != 0
    rc, _ = plan_text(lib, _args(N=320, K=256, ntaps=1, lda=256, ldw=256, ldc=320, C2=None, N1=0, A2=5 << 36, lda2=256))
    assert rc != 0
    # a launch without either field plans as before
    rc, text = plan_text(lib, _args(N=256, C2=None, N1=0))
    assert rc == 0 and plan_lines(text)[0][0] == "gemm_kernel<bf16,64,64,2,2>"
