"""The ResnetBlock1D fold (CVFT_RESNET_FOLD): block1's k = 3 convolution and the 1x1 shortcut as one tap-GEMM launch each way,
the sum h + shortcut inside block2's GroupNorm + Mish launch, and one GEMM for the decoder's time projections.

Every comparison has a yardstick that is not the code under test: the separate launches the fold replaces (bit equality where
the arithmetic per element is the same), or torch in fp64 on the same stored operands, with the separate path's own error
against fp64 as the scale of the bound.  err(a) below is the relative Frobenius error of a against the fp64 result."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
# B = 2 with one short utterance; T = 37 is no multiple of the 64-row tile; with T = 130 a tile boundary (row 64, row 128) falls
# inside an utterance, so the taps t - 1 / t + 1 of its edge rows come from the neighbouring tile's rows
SHAPES = [(37, [37, 21], 320, 256), (37, [37, 21], 256, 256), (130, [130, 77], 320, 256)]


def HFmod():
    from cosyvoice_lora_finetune_framework_amd.hipops import functional as HF
    return HF


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def err(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / (ref.norm() + 1e-300))


def shifted(x, o):
    """x [B, T, C] -> rows t + o, zero outside [0, T)"""
    T = x.shape[1]
    y = torch.zeros_like(x)
    lo, hi = max(0, -o), min(T, T - o)
    y[:, lo:hi] = x[:, lo + o:hi + o]
    return y


def same_or_no_worse(fold, sep, ref, margin, what):
    """bit equality, else the fp64 rule: err(fold) <= margin * err(sep)"""
    ef, es = err(fold, ref), err(sep, ref)
    print(f"{what}: equal={torch.equal(fold, sep)} err_fold={ef:.3e} err_sep={es:.3e}")
    assert torch.equal(fold, sep) or ef <= margin * es, (what, ef, es)


@pytest.fixture(scope="module")
def convs():
    """per shape: bf16 operands on the device, the pack, and fp64 copies of what is stored"""
    HF = HFmod()
    out = {}
    for T, lens, Cin, N in SHAPES:
        B = len(lens)
        c3, c1 = torch.nn.Conv1d(Cin, N, 3, padding=1), torch.nn.Conv1d(Cin, N, 1)
        g = torch.Generator().manual_seed(Cin + T)
        with torch.no_grad():
            for c in (c3, c1):
                c.weight.copy_(torch.randn(c.weight.shape, generator=g) * (2.0 / (c.weight.shape[1] * c.weight.shape[2])) ** 0.5)
                c.bias.copy_(torch.randn(c.bias.shape, generator=g) * 0.1)
        c3, c1 = c3.to(DEV), c1.to(DEV)
        out[(T, Cin)] = dict(B=B, T=T, Cin=Cin, N=N, c3=c3, c1=c1, pair=HF.ConvPairPack(c3, c1, BF),
                             p3=HF.ConvPack(c3.weight, c3.bias, BF), p1=HF.ConvPack(c1.weight, c1.bias, BF),
                             length=torch.tensor(lens, dtype=torch.int32, device=DEV),
                             x=rnd(B * T, Cin, seed=1).to(DEV, BF), dh=rnd(B * T, N, seed=2).to(DEV, BF),
                             dr=rnd(B * T, N, seed=3).to(DEV, BF))
    return out


@pytest.mark.parametrize("T,lens,Cin,N", SHAPES)
def test_two_output_launch_equals_the_two_launches(convs, T, lens, Cin, N):
    """C and C2 of the two-output launch against the two cvft_gemm calls it replaces (k = 3 taps with the in_len mask; the 1x1
    with the same mask), padded rows included.  Each element is the same chain of 64-wide k-tiles in the same order -- the
    shortcut tiles skip the other taps' k-tiles instead of adding zeros -- so the results are expected bit-equal.  Were they not,
    the fp64 rule applies with margin 1.1: both paths round the same fp32 sums to bf16 once, so a different summation order could
    only move single roundings (an fp32 ulp flipping a bf16 rounding), far below 10 % of the rounding error itself.
    Measured on MI355X: bit-equal in all three shapes (err_fold = err_sep = 1.64e-3 .. 1.69e-3)."""
    HF = HFmod()
    c = convs[(T, Cin)]
    B, length = c["B"], c["length"]
    geo = HF.Geo(Tm=T, Tin=T, Tout=T, taps=(-1, 0, 1))
    h_sep = HF.gemm(c["x"], c["p3"].Wf, bias=c["p3"].bias, geo=geo, nb=B, in_len=length)
    r_sep = HF.gemm(c["x"], c["p1"].Wf, bias=c["p1"].bias, geo=HF.Geo(Tm=T, Tin=T, Tout=T), nb=B, in_len=length)
    h = torch.full((B * T, N), float("nan"), dtype=BF, device=DEV)
    r = torch.full((B * T, N), float("nan"), dtype=BF, device=DEV)
    HF.gemm(c["x"], c["pair"].Wf, K=Cin, bias=c["pair"].bias, geo=geo, nb=B, in_len=length, out=h, out2=r, bias2=c["pair"].bias2)
    assert HF.lib().cvft_gemm_last_kernel().decode() == "gemm_kernel<bf16,64,64,2,2>,two_out"
    mask = (torch.arange(T, device=DEV)[None, :] < length[:, None]).double()[:, :, None]
    xm = c["x"].double().reshape(B, T, Cin) * mask
    w3, w1 = c["p3"].Wf.double(), c["p1"].Wf.double()
    h64 = sum(shifted(xm, o) @ w3[:, j * Cin:(j + 1) * Cin].t() for j, o in enumerate((-1, 0, 1))) + c["p3"].bias.double()
    r64 = xm @ w1.t() + c["p1"].bias.double()
    same_or_no_worse(h, h_sep, h64.reshape(B * T, N), 1.1, "C")
    same_or_no_worse(r, r_sep, r64.reshape(B * T, N), 1.1, "C2")
    # rows at or beyond in_len of the shortcut: the bias, as res_conv(x * mask) gives
    dead = (torch.arange(T, device=DEV)[None, :] >= length[:, None]).reshape(B * T)
    assert torch.equal(r[dead], c["p1"].bias.to(BF).expand(int(dead.sum()), N))


@pytest.mark.parametrize("T,lens,Cin,N", SHAPES)
def test_two_operand_dgrad_against_fp64(convs, T, lens, Cin, N):
    """dx = sum_taps dh[t + tau] W3^T_tau + dr[t] W1^T as one four-tap launch (the fourth tap on the second A operand, cvft.h A2) against the
    pair it replaces: the 1x1 dgrad whose bf16 result is parked, then the k = 3 dgrad adding it in its epilogue.  The fold moves a
    rounding (the parked tensor's disappears), so the yardstick is fp64 on the stored operands and the bound is the separate
    path's own error times 1.1: the folded launch forms the same fp32 MFMA sums and rounds once where the pair rounds twice, so its
    error can only be lower in expectation; 10 % covers the sampling scatter of a Frobenius error over >= 2 * 37 * 256 elements
    (about 1 %) and fp32 summation order (2^-24 against bf16's 2^-9).  dx rows at or beyond in_len are zero either way.
    Measured on MI355X: err_fold 1.67e-3 against err_sep 2.04e-3 .. 2.06e-3 in all three shapes."""
    HF = HFmod()
    c = convs[(T, Cin)]
    B, length = c["B"], c["length"]
    parked = HF.gemm(c["dr"], c["p1"].Wb[0], geo=HF.Geo(Tm=T, Tin=T, Tout=T), nb=B, out_len=length)
    dx_sep = HF.gemm(c["dh"], c["p3"].Wb[0], geo=HF.Geo(Tm=T, Tin=T, Tout=T, taps=(-1, 0, 1)), nb=B, out_len=length, residual=parked)
    dx = HF.gemm(c["dh"], c["pair"].Wb, N=Cin, K=N, geo=HF.Geo(Tm=T, Tin=T, Tout=T, taps=(-1, 0, 1, 0)), nb=B, out_len=length,
                 x2=c["dr"])
    assert HF.lib().cvft_gemm_last_kernel().decode() == "gemm_kernel<bf16,64,64,2,2>,two_in"
    mask = (torch.arange(T, device=DEV)[None, :] < length[:, None]).double()[:, :, None]
    dh, dr = c["dh"].double().reshape(B, T, N), c["dr"].double().reshape(B, T, N)
    wb3, wb1 = c["p3"].Wb[0].double(), c["p1"].Wb[0].double()
    ref = (sum(shifted(dh, o) @ wb3[:, j * N:(j + 1) * N].t() for j, o in enumerate((-1, 0, 1))) + dr @ wb1.t()) * mask
    ref = ref.reshape(B * T, Cin)
    ef, es = err(dx, ref), err(dx_sep, ref)
    print(f"dgrad T={T} Cin={Cin}: err_fold={ef:.3e} err_sep={es:.3e}")
    assert ef <= 1.1 * es, (ef, es)
    dead = (torch.arange(T, device=DEV)[None, :] >= length[:, None]).reshape(B * T)
    assert float(dx[dead].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("B,T,Te,G,Cn", [(2, 37, 37, 8, 256), (2, 40, 29, 8, 256), (2, 37, 30, 1, 1024)])
def test_groupnorm_mish_with_residual(dtype, B, T, Te, G, Cn):
    """out = mish(gn(x)) * mask + add + res against the launch without res plus an add in fp32, on the one-launch kernel and (C / G
    = 1024: the slab does not fit a block) on the statistics + apply pair; `add` a column slice of a wider tensor, read in place.
    fp32: the same fp32 sum, bit-equal.  bf16: the launch rounds o + res once where the yardstick holds rn(o), so
    |out - (rn(o) + res)| <= 2^-8 (|o + res| + |o|): two roundings of half an ulp each, and half an ulp of bf16's 8-bit significand
    is at most 2^-8 of the value (1 % on top for o against rn(o) inside the bound itself).  With t_true < T (the
    shape-bucket case) the padding frames hold NaN in x: live frames are bit-equal to the clean run, padding frames are res itself;
    the gradient of res is dy, bit for bit, and dx is that of the launch without res."""
    HF = HFmod()
    lens = torch.tensor([Te, max(1, Te - 9)], dtype=torch.int32, device=DEV)
    te = None if Te == T else torch.tensor([Te], dtype=torch.int32, device=DEV)
    g, b = (1 + 0.1 * rnd(Cn, seed=2)).to(DEV), (0.1 * rnd(Cn, seed=3)).to(DEV)
    x0 = (rnd(B, T, Cn, seed=1) + 0.2).to(DEV, dtype)
    wide = rnd(B, 3 * Cn, seed=4).to(DEV, dtype)
    add = wide[:, Cn:2 * Cn]
    res0 = rnd(B * T, Cn, seed=5).to(DEV, dtype)
    gy = rnd(B * T, Cn, seed=6).to(DEV, dtype)
    outs = []
    for poison in ((False, True) if te is not None else (False,)):
        x = x0.clone()
        if poison:
            x[:, Te:, :] = float("nan")
        xd, xe = x.reshape(B * T, Cn).clone().requires_grad_(True), x.reshape(B * T, Cn).clone().requires_grad_(True)
        res = res0.clone().requires_grad_(True)
        y = HF.groupnorm_mish(xd, g, b, B, T, G, 1e-5, lens, add, True, t_eff=te, res=res)
        y0 = HF.groupnorm_mish(xe, g, b, B, T, G, 1e-5, lens, add.contiguous(), True, t_eff=te)
        y.backward(gy)
        y0.backward(gy)
        assert torch.equal(res.grad, gy)
        live = slice(0, Te)
        assert torch.equal(xd.grad.reshape(B, T, Cn)[:, live], xe.grad.reshape(B, T, Cn)[:, live])
        yl, y0l, rl = (t.detach().reshape(B, T, Cn)[:, live].float() for t in (y, y0, res0))
        assert torch.isfinite(yl).all()
        ref = y0l + rl
        if dtype == torch.float32:
            assert torch.equal(yl, ref)
        else:
            assert bool(((yl - ref).abs() <= 2.0 ** -8 * (ref.abs() + y0l.abs()) * 1.01 + 1e-37).all())
        if te is not None:
            assert torch.equal(y.detach().reshape(B, T, Cn)[:, Te:], res0.reshape(B, T, Cn)[:, Te:])
        outs.append(y.detach().reshape(B, T, Cn)[:, live].clone())
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1])


def _block(Cin, Cout, Ct=64, seed=4):
    from cosyvoice_lora_finetune_framework_amd.modules import ResnetBlock1D
    torch.manual_seed(seed)
    blk = ResnetBlock1D(Cin, Cout, Ct).to(DEV)
    for p in blk.parameters():
        p.requires_grad_(False)
    return blk


def _run_block(blk, fold: bool, x0, temb_mish, g, B, T, length):
    """(y, dx, libcvft calls) of one forward + backward with the fold on / off"""
    from cosyvoice_lora_finetune_framework_amd.hipops import binding as cb
    x = x0.clone().requires_grad_(True)
    n0 = cb.CALLS
    y = blk(x, B, T, length, temb_mish, fold=fold)          # (as the decoder calls it under CVFT_RESNET_FOLD=1 / =0)
    y.backward(g)
    calls = cb.CALLS - n0
    torch.cuda.synchronize()
    return y.detach().clone(), x.grad.clone(), calls


def _block_fp64(blk, x0, temb_mish, g, B, T, length):
    Cin, Cout = x0.shape[1], g.shape[1]
    xr = x0.double().reshape(B, T, Cin).transpose(1, 2).clone().requires_grad_(True)
    mask = (torch.arange(T, device=DEV)[None, :] < length[:, None]).double()[:, None, :]
    W = lambda m: (m.weight.double(), m.bias.double())                                          # noqa: E731

    def block1d(b1d, h):
        conv, gn = b1d.block[0], b1d.block[1]
        h = F.conv1d(h * mask, *W(conv), padding=1)
        return F.mish(F.group_norm(h, gn.num_groups, gn.weight.double(), gn.bias.double(), gn.eps)) * mask
    h = block1d(blk.block1, xr) + F.linear(temb_mish.double(), *W(blk.mlp[1]))[:, :, None]
    yr = block1d(blk.block2, h) + F.conv1d(xr * mask, *W(blk.res_conv))
    yr.backward(g.double().reshape(B, T, Cout).transpose(1, 2))
    return yr.detach().transpose(1, 2).reshape(B * T, Cout), xr.grad.transpose(1, 2).reshape(B * T, Cin)


@pytest.mark.parametrize("T,lens,Cin,Cout", SHAPES)
def test_block_folded_against_separate_launches(T, lens, Cin, Cout):
    """ResnetBlock1D, fold on against fold off, same seeded inputs, bf16; the yardstick is torch fp64 on the module's own math
    (the module's weights are fp32 and both paths round them to bf16 alike, so that part of the error is common).
    Output: both paths round twice on the way to y = h + r.  The separate launches round h (block2's output) and then the sum;
    the fold rounds r (the shortcut) and then the sum.  Rounding errors scale with the rounded value, so err_fold / err_sep is at
    most sqrt((r^2 + y^2) / (h^2 + y^2)) in rms terms: with this initialisation rms(r) = 1.4 (kaiming, unit input), rms(h) = 0.6
    and y^2 = h^2 + r^2 that is 1.26; the bound is 1.3 x the separate path's error: the argued worst case plus 3 % for the
    sampling scatter of a Frobenius error over these few thousand elements (the three shapes scatter by that much).
    dx (which the block-output gradient reaches through the shortcut tap and through block2): every backward launch before the
    last sees bit-identical operands on both paths -- the saved tensors are the same -- and the last is the two-operand dgrad, one
    rounding instead of two: bound 1.1 x the separate path's error, as in the kernel-level test.
    The folded forward + backward makes 2 libcvft calls fewer (the shortcut's forward GEMM and its dgrad).
    Measured on MI355X (T = 37, 320 -> 256): y err_fold 3.74e-3 / err_sep 3.85e-3; dx err_fold 4.07e-3 / err_sep 4.18e-3; the
    other two shapes within 3 % of these."""
    blk = _block(Cin, Cout)
    B = len(lens)
    length = torch.tensor(lens, dtype=torch.int32, device=DEV)
    x0 = rnd(B * T, Cin, seed=1).to(DEV, BF)
    temb_mish = F.mish(rnd(B, 64, seed=2)).to(DEV, BF)
    g = rnd(B * T, Cout, seed=3).to(DEV, BF)
    yf, gf, nf = _run_block(blk, True, x0, temb_mish, g, B, T, length)
    ys, gs, ns = _run_block(blk, False, x0, temb_mish, g, B, T, length)
    assert ns - nf == 2, (ns, nf)
    yr, gr = _block_fp64(blk, x0, temb_mish, g, B, T, length)
    print(f"block T={T} Cin={Cin}: y err_fold={err(yf, yr):.3e} err_sep={err(ys, yr):.3e}; dx err_fold={err(gf, gr):.3e} err_sep={err(gs, gr):.3e}")
    assert err(yf, yr) <= 1.3 * err(ys, yr)
    assert err(gf, gr) <= 1.1 * err(gs, gr)
    dead = (torch.arange(T, device=DEV)[None, :] >= length[:, None]).reshape(B * T)
    assert float(gf[dead].abs().max()) == 0.0 and torch.equal(yf[dead], ys[dead])


def test_block_falls_back_bit_for_bit():
    """fp32 blocks, and a block whose conv is not a plain nn.Conv1d (here: a subclass standing in for an adapter), take the
    separate launches whatever the switch says: same results bit for bit, same number of libcvft calls."""
    T, lens, Cin, Cout = 37, [37, 21], 320, 256
    B = len(lens)
    length = torch.tensor(lens, dtype=torch.int32, device=DEV)
    temb = F.mish(rnd(B, 64, seed=2))
    for dtype, wrap in ((torch.float32, False), (BF, True)):
        blk = _block(Cin, Cout)
        if wrap:
            class Wrapped(torch.nn.Conv1d):
                pass
            blk.res_conv.__class__ = Wrapped
        x0, g = rnd(B * T, Cin, seed=1).to(DEV, dtype), rnd(B * T, Cout, seed=3).to(DEV, dtype)
        yf, gf, nf = _run_block(blk, True, x0, temb.to(DEV, dtype), g, B, T, length)
        ys, gs, ns = _run_block(blk, False, x0, temb.to(DEV, dtype), g, B, T, length)
        assert nf == ns and torch.equal(yf, ys) and torch.equal(gf, gs)


def test_block_with_trainable_time_projection_keeps_its_own_launch():
    """A block whose mlp[1] requires grad is not stackable, so the decoder hands it no `add` and it runs its own hip_linear launch
    (under no_grad, as before): fold off, its output and dx equal the frozen block's separate launches bit for bit, with the same
    number of libcvft calls; fold on, they equal the frozen block's folded launches bit for bit."""
    T, lens, Cin, Cout = 37, [37, 21], 320, 256
    B = len(lens)
    length = torch.tensor(lens, dtype=torch.int32, device=DEV)
    temb = F.mish(rnd(B, 64, seed=2)).to(DEV, BF)
    x0, g = rnd(B * T, Cin, seed=1).to(DEV, BF), rnd(B * T, Cout, seed=3).to(DEV, BF)
    blk = _block(Cin, Cout)
    assert blk.time_proj_stackable()
    frozen = {fold: _run_block(blk, fold, x0, temb, g, B, T, length) for fold in (False, True)}
    blk.mlp[1].weight.requires_grad_(True)
    assert not blk.time_proj_stackable()
    for fold in (False, True):
        y, dx, n = _run_block(blk, fold, x0, temb, g, B, T, length)
        assert n == frozen[fold][2] and torch.equal(y, frozen[fold][0]) and torch.equal(dx, frozen[fold][1])
    assert blk.mlp[1].weight.grad is None


@pytest.fixture(scope="module")
def decoder():
    from cosyvoice_lora_finetune_framework_amd.modules import ConditionalDecoder
    torch.manual_seed(0)
    dec = ConditionalDecoder(320, 80, channels=(256, 256), num_mid_blocks=2, n_blocks=1).to(DEV)
    for p in dec.parameters():
        p.requires_grad_(False)
    return dec


def test_stacked_time_projection_equals_the_per_block_linears(decoder):
    """One GEMM [B, 1024] x [1024, 6 * 256] against the six hip_linear(mlp[1], .) launches it replaces: each block's column
    slice, read in place.  Same K walk per element, expected bit-equal; were it not, the fp64 rule with margin 1.1 as in the
    forward kernel test (one bf16 rounding of the same fp32 sums either way).  Measured on MI355X: bit-equal, all six slices."""
    HF = HFmod()
    from cosyvoice_lora_finetune_framework_amd import modules as M
    B = 2
    temb_mish = F.mish(rnd(B, 1024, seed=7)).to(DEV, BF)
    keep = HF.RESNET_FOLD_TEMB
    HF.RESNET_FOLD_TEMB = True
    try:
        with torch.no_grad():
            adds = decoder._stacked_time_proj(temb_mish)
            resnets = decoder._resnets()
            assert len(adds) == len(resnets) == 6 and all(a is not None for a in adds)
            base = adds[0]._base if adds[0]._base is not None else adds[0]
            assert all(a.data_ptr() == base.data_ptr() + 2 * 256 * i and a.stride(0) == 6 * 256 for i, a in enumerate(adds))
            for i, (r, a) in enumerate(zip(resnets, adds)):
                sep = M.hip_linear(r.mlp[1], temb_mish)
                ref = temb_mish.double() @ r.mlp[1].weight.to(BF).double().t() + r.mlp[1].bias.double()
                same_or_no_worse(a, sep, ref, 1.1, f"time projection {i}")
    finally:
        HF.RESNET_FOLD_TEMB = keep


def test_stacked_time_projection_leaves_trainable_and_fp32_blocks_alone(decoder):
    """A block whose mlp[1] requires grad computes its own projection (its slot is None, the others are stacked without it); an
    fp32 decoder stacks nothing; with the switch off nothing is stacked."""
    HF = HFmod()
    B = 2
    temb_mish = F.mish(rnd(B, 1024, seed=7)).to(DEV, BF)
    keep = HF.RESNET_FOLD_TEMB
    lin = decoder._resnets()[2].mlp[1]
    try:
        HF.RESNET_FOLD_TEMB = True
        lin.weight.requires_grad_(True)
        with torch.no_grad():
            adds = decoder._stacked_time_proj(temb_mish)
            assert [a is None for a in adds] == [False, False, True, False, False, False]
            assert adds[3].stride(0) == 5 * 256
            assert all(a is None for a in decoder._stacked_time_proj(temb_mish.float()))
            HF.RESNET_FOLD_TEMB = False
            assert all(a is None for a in decoder._stacked_time_proj(temb_mish))
    finally:
        lin.weight.requires_grad_(False)
        HF.RESNET_FOLD_TEMB = keep
