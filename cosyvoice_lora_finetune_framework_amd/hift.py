"""The HiFT vocoder on HIP: mel -> waveform (hifigan/generator.py HiFTGenerator.inference with the ConvRNNF0Predictor
of hifigan/f0_predictor.py), the 22 050 Hz CosyVoice-300M configuration, inference only.

``HiFTGenerator`` / ``ConvRNNF0Predictor`` are parameter containers with the reference's constructor arguments and
state-dict keys (weight-normed convolutions as ``<name>.parametrizations.weight.original0`` (g) / ``original1`` (v); the
legacy ``weight_g`` / ``weight_v`` spelling is accepted at load time).  Weight norm is folded once per weight dtype
(``PackedHiFT``, fp32 parity path or bf16 product path) into the tap-major ``[k][C_out][C_in]`` layout of
``cvft_hift_conv``.  Activations are channel-last fp32 rows ``[B*T, C]``.  Everything runs through csrc/hift.hip; there
is no eager fallback.

    f0      = |classifier(condnet(mel))|                         5 x cvft_hift_conv (k 3, ELU) + cvft_hift_conv_small
    source  = tanh(linear(harmonics of f0 + noise))              cvft_hift_scan (fp64 phase sum) + cvft_hift_source
    decode  = STFT(source) -> conv_pre -> 2 x (leaky-ReLU, transposed conv as 8 phase launches, + source branch,
              mean of 3 residual blocks) -> conv_post -> ISTFT   cvft_hift_stft / _conv / _conv_small / _istft
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
from torch.nn.utils.parametrizations import weight_norm

from .hipops.binding import BF16, F32, HiftConvArgs, check, lib, ptr, stream

PRE_NONE, PRE_SNAKE, PRE_LEAKY = 0, 1, 2
MAX_SPAN = 50         # HC_SPAN (csrc/hift.hip): (k - 1) * d of the widest convolution


# ---------------------------------------------------------------------------------------------- containers
class Snake(nn.Module):
    def __init__(self, channels: int):
        super().__init__()
        self.alpha = nn.Parameter(torch.ones(channels))


class ResBlock(nn.Module):
    def __init__(self, channels: int = 512, kernel_size: int = 3, dilations=(1, 3, 5)):
        super().__init__()
        self.kernel_size, self.dilations = kernel_size, tuple(dilations)
        pad = lambda d: (kernel_size * d - d) // 2          # noqa: E731
        self.convs1 = nn.ModuleList(weight_norm(nn.Conv1d(channels, channels, kernel_size, 1, dilation=d, padding=pad(d)))
                                    for d in dilations)
        self.convs2 = nn.ModuleList(weight_norm(nn.Conv1d(channels, channels, kernel_size, 1, padding=pad(1)))
                                    for _ in dilations)
        self.activations1 = nn.ModuleList(Snake(channels) for _ in dilations)
        self.activations2 = nn.ModuleList(Snake(channels) for _ in dilations)


class _Source(nn.Module):
    def __init__(self, harmonics: int):
        super().__init__()
        self.l_linear = nn.Linear(harmonics, 1)


class ConvRNNF0Predictor(nn.Module):
    def __init__(self, num_class: int = 1, in_channels: int = 80, cond_channels: int = 512):
        super().__init__()
        if num_class != 1:
            raise NotImplementedError(f"ConvRNNF0Predictor: num_class={num_class} (only 1 is built)")
        if cond_channels % 64:
            raise NotImplementedError(f"ConvRNNF0Predictor: cond_channels={cond_channels} is not a multiple of 64")
        self.num_class, self.in_channels, self.cond_channels = num_class, in_channels, cond_channels
        layers: List[nn.Module] = []
        for i in range(5):
            layers += [weight_norm(nn.Conv1d(in_channels if i == 0 else cond_channels, cond_channels, 3, padding=1)), nn.ELU()]
        self.condnet = nn.Sequential(*layers)
        self.classifier = nn.Linear(cond_channels, num_class)


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """w = g * v / ||v||, the norm over every dim but 0 (torch._weight_norm(v, g, 0)); for a ConvTranspose1d dim 0 is
    the input channel."""
    n = v.float().flatten(1).norm(dim=1).reshape(-1, *([1] * (v.dim() - 1)))
    return v.float() * (g.float() / n)


def _folded(conv: nn.Module) -> torch.Tensor:
    p = conv.parametrizations.weight
    return fold_weight_norm(p.original0.detach(), p.original1.detach())


def _legacy_keys(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight_g"):
            k = k[:-len("weight_g")] + "parametrizations.weight.original0"
        elif k.endswith(".weight_v"):
            k = k[:-len("weight_v")] + "parametrizations.weight.original1"
        out[k] = v
    return out


# ---------------------------------------------------------------------------------------------- ops
class ConvPack:
    """One convolution (or one output phase of a transposed one) in cvft_hift_conv's layout."""

    def __init__(self, taps: torch.Tensor, offsets, bias: Optional[torch.Tensor], wdtype: torch.dtype):
        # taps [ntaps, Cout, Cin] fp32
        nt, co, ci = taps.shape
        self.Cout, self.CoutP, self.Cin = co, -(-co // 64) * 64, -(-ci // 64) * 64
        W = torch.zeros((nt, self.CoutP, self.Cin), dtype=torch.float32, device=taps.device)
        W[:, :co, :ci] = taps
        self.W = W.to(wdtype).contiguous()
        self.bias = bias.detach().float().contiguous() if bias is not None else None
        self.offsets = [int(o) for o in offsets]
        self.dtype = BF16 if wdtype == torch.bfloat16 else F32
        if max(self.offsets) - min(self.offsets) > MAX_SPAN or nt > 11:
            raise NotImplementedError(f"convolution with {nt} taps spanning {max(self.offsets) - min(self.offsets)} rows "
                                      f"(at most 11 taps, span {MAX_SPAN})")


def pack_conv1d(w: torch.Tensor, bias, dilation: int, wdtype) -> ConvPack:
    """w [Cout, Cin, k] of a 'same'-padded stride-1 Conv1d."""
    k = w.shape[2]
    return ConvPack(w.permute(2, 0, 1), [(j - (k - 1) // 2) * dilation for j in range(k)], bias, wdtype)


def pack_conv_transpose_k16s8(w: torch.Tensor, bias, wdtype) -> List[ConvPack]:
    """w [Cin, Cout, 16] of ConvTranspose1d(k 16, s 8, p 4): output 8q + ph = x[q] w[ph+4] + (x[q-1] w[ph+12] if ph < 4
    else x[q+1] w[ph-4])."""
    packs = []
    for ph in range(8):
        k2, off2 = (ph + 12, -1) if ph < 4 else (ph - 4, 1)
        taps = torch.stack([w[:, :, ph + 4].t(), w[:, :, k2].t()])
        packs.append(ConvPack(taps, [0, off2], bias, wdtype))
    return packs


def hift_conv(x: torch.Tensor, pk: ConvPack, B: int, Tin: int, pre: int = PRE_NONE, alpha=None, slope: float = 0.0,
              elu: bool = False, res=None, res2=None, accum: bool = False, scale: float = 1.0, out=None,
              Tq: Optional[int] = None, Tout: Optional[int] = None, out_stride: int = 1, out_off: int = 0) -> torch.Tensor:
    """x [B*Tin, >= pk.Cin] fp32 rows -> y [B*Tout, pk.Cout] (include/cvft.h, cvft_hift_conv)."""
    Tq = Tin if Tq is None else Tq
    Tout = Tq if Tout is None else Tout
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == B * Tin and x.shape[1] >= pk.Cin
    if out is None:
        out = torch.empty((B * Tout, pk.Cout), dtype=torch.float32, device=x.device)
    assert out.shape == (B * Tout, pk.Cout) and out.stride(1) == 1
    a = HiftConvArgs()
    a.dtype, a.B, a.Tin, a.Tq, a.Tout, a.out_stride, a.out_off = pk.dtype, B, Tin, Tq, Tout, out_stride, out_off
    a.Cin, a.Cout, a.CoutP, a.ntaps = pk.Cin, pk.Cout, pk.CoutP, len(pk.offsets)
    for j, o in enumerate(pk.offsets):
        a.tap_off[j] = o
    a.x, a.ldx, a.W, a.bias = ptr(x), x.stride(0), ptr(pk.W), ptr(pk.bias)
    a.pre, a.alpha, a.slope, a.elu = pre, ptr(alpha), float(slope), int(elu)
    a.res, a.ldr = ptr(res), (res.stride(0) if res is not None else 0)
    a.res2, a.ldr2 = ptr(res2), (res2.stride(0) if res2 is not None else 0)
    a.accum, a.scale, a.y, a.ldy = int(accum), float(scale), ptr(out), out.stride(0)
    check(lib().cvft_hift_conv(a, stream()), "cvft_hift_conv")
    return out


def conv_small(x: torch.Tensor, W: torch.Tensor, bias, B: int, Tin: int, Tout: int, stride: int = 1, pad: int = 0,
               absval: bool = False) -> torch.Tensor:
    """x [B*Tin, >= Cin] fp32, W [k, Cin, Cout] fp32 -> [B*Tout, Cout] (cvft_hift_conv_small)."""
    k, Cin, Cout = W.shape
    assert x.dtype == torch.float32 and x.stride(1) == 1 and W.is_contiguous() and x.shape[0] == B * Tin
    y = torch.empty((B * Tout, Cout), dtype=torch.float32, device=x.device)
    check(lib().cvft_hift_conv_small(B, Tin, Tout, Cin, Cout, k, stride, pad, ptr(x), x.stride(0), ptr(W), ptr(bias),
                                     int(absval), ptr(y), Cout, stream()), "cvft_hift_conv_small")
    return y


def scan(x: torch.Tensor, L: int, rep: int = 1, div: float = 1.0) -> torch.Tensor:
    """x [R, ceil(L / rep)] fp32 -> fp32(fp64 running sum of x[r, n // rep] / div) [R, L]; the division is the correctly
    rounded fp32 one (torch's GPU division by a scalar multiplies by the reciprocal, which is 1 ulp off for some
    inputs -- over 35 000 samples that moved the phase by an ulp of the sum)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and x.shape[1] == -(-L // rep)
    y = torch.empty((x.shape[0], L), dtype=torch.float32, device=x.device)
    check(lib().cvft_hift_scan(x.shape[0], L, rep, ptr(x), float(div), ptr(y), stream()), "cvft_hift_scan")
    return y


def stft(s: torch.Tensor) -> torch.Tensor:
    """s [B, L] fp32 -> [B*(L/4+1), 18] real | imag (n_fft 16, hop 4, periodic Hann, centre reflect padding)."""
    assert s.dtype == torch.float32 and s.dim() == 2 and s.is_contiguous()
    B, L = s.shape
    out = torch.empty((B * (L // 4 + 1), 18), dtype=torch.float32, device=s.device)
    check(lib().cvft_hift_stft(B, L, ptr(s), ptr(out), stream()), "cvft_hift_stft")
    return out


def istft(x: torch.Tensor, B: int, limit: float = 0.99, want_mag: bool = False):
    """x [B*F, 18] (log-magnitude | phase argument) -> wav [B, 4*(F-1)] clamped to +-limit (, clipped magnitudes)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] % B == 0 and x.shape[1] >= 18
    F = x.shape[0] // B
    wav = torch.empty((B, 4 * (F - 1)), dtype=torch.float32, device=x.device)
    mag = torch.empty((B * F, 9), dtype=torch.float32, device=x.device) if want_mag else None
    check(lib().cvft_hift_istft(B, F, ptr(x), x.stride(0), float(limit), ptr(wav), ptr(mag), stream()), "cvft_hift_istft")
    return (wav, mag) if want_mag else wav


# ---------------------------------------------------------------------------------------------- packed weights
class PackedResBlock:
    def __init__(self, rb: ResBlock, wdtype):
        f32 = lambda t: t.detach().float().contiguous()          # noqa: E731
        self.c1 = [pack_conv1d(_folded(c), c.bias, d, wdtype) for c, d in zip(rb.convs1, rb.dilations)]
        self.c2 = [pack_conv1d(_folded(c), c.bias, 1, wdtype) for c in rb.convs2]
        self.a1 = [f32(a.alpha) for a in rb.activations1]
        self.a2 = [f32(a.alpha) for a in rb.activations2]

    def run(self, x, B, T, out=None, accum=False, scale=1.0, res2=None):
        """ResBlock.forward of x [B*T, C] (left untouched); the last convolution's epilogue also adds res2, adds into
        `out` (accum) and scales."""
        n = len(self.c1)
        h = x
        for i in range(n):
            t = hift_conv(h, self.c1[i], B, T, pre=PRE_SNAKE, alpha=self.a1[i])
            last = i == n - 1
            h = hift_conv(t, self.c2[i], B, T, pre=PRE_SNAKE, alpha=self.a2[i], res=h,
                          res2=res2 if last else None, accum=accum and last, scale=scale if last else 1.0,
                          out=out if last else (h if i > 0 else None))
        return h


class PackedHiFT:
    """The weights of a HiFTGenerator (+ its f0 predictor) folded and packed once for one weight dtype."""

    def __init__(self, m: "HiFTGenerator", wdtype: torch.dtype):
        self.wdtype = wdtype
        f32 = lambda t: t.detach().float().contiguous()          # noqa: E731
        fp = m.f0_predictor
        self.f0_convs = [pack_conv1d(_folded(fp.condnet[2 * i]), fp.condnet[2 * i].bias, 1, wdtype) for i in range(5)]
        self.f0_cls_w = f32(fp.classifier.weight.t()).reshape(1, fp.cond_channels, 1)
        self.f0_cls_b = f32(fp.classifier.bias)
        self.lw, self.lb = f32(m.m_source.l_linear.weight).reshape(-1), f32(m.m_source.l_linear.bias)
        self.conv_pre = pack_conv1d(_folded(m.conv_pre), m.conv_pre.bias, 1, wdtype)
        self.ups = [pack_conv_transpose_k16s8(_folded(u), u.bias, wdtype) for u in m.ups]
        self.down_w = [f32(d.weight.permute(2, 1, 0)) for d in m.source_downs]            # [k, 18, C]
        self.down_b = [f32(d.bias) for d in m.source_downs]
        self.src_rb = [PackedResBlock(rb, wdtype) for rb in m.source_resblocks]
        self.rbs = [PackedResBlock(rb, wdtype) for rb in m.resblocks]
        self.conv_post = pack_conv1d(_folded(m.conv_post), m.conv_post.bias, 1, wdtype)


# ---------------------------------------------------------------------------------------------- the generator
class HiFTGenerator(nn.Module):
    def __init__(self, in_channels: int = 80, base_channels: int = 512, nb_harmonics: int = 8, sampling_rate: int = 22050,
                 nsf_alpha: float = 0.1, nsf_sigma: float = 0.003, nsf_voiced_threshold: float = 10,
                 upsample_rates=(8, 8), upsample_kernel_sizes=(16, 16), istft_params=None,
                 resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)),
                 source_resblock_kernel_sizes=(7, 11), source_resblock_dilation_sizes=((1, 3, 5), (1, 3, 5)),
                 lrelu_slope: float = 0.1, audio_limit: float = 0.99, f0_predictor: Optional[nn.Module] = None,
                 dtype: torch.dtype = torch.float32):
        super().__init__()
        istft_params = dict(istft_params) if istft_params is not None else {"n_fft": 16, "hop_len": 4}
        if sampling_rate != 22050:
            raise NotImplementedError(f"sampling_rate={sampling_rate}: only the 22 050 Hz SourceModuleHnNSF / SineGen path "
                                      f"is built (not SourceModuleHnNSF2 / SineGen2)")
        if istft_params != {"n_fft": 16, "hop_len": 4}:
            raise NotImplementedError(f"istft_params={istft_params}: only n_fft 16 / hop_len 4 is built")
        if list(upsample_rates) != [8, 8] or list(upsample_kernel_sizes) != [16, 16]:
            raise NotImplementedError(f"upsample_rates={list(upsample_rates)} / upsample_kernel_sizes="
                                      f"{list(upsample_kernel_sizes)}: only [8, 8] / [16, 16] is built")
        if base_channels % 256:
            raise NotImplementedError(f"base_channels={base_channels}: every stage's channel count must be a multiple of 64")
        if (nsf_alpha, nsf_sigma) != (0.1, 0.003) or nb_harmonics + 1 > 16:
            raise NotImplementedError(f"nsf_alpha={nsf_alpha} / nsf_sigma={nsf_sigma} / nb_harmonics={nb_harmonics}: only "
                                      f"0.1 / 0.003 / <= 15 is built")
        for ks, ds in zip(list(resblock_kernel_sizes) + list(source_resblock_kernel_sizes),
                          list(resblock_dilation_sizes) + list(source_resblock_dilation_sizes)):
            if ks % 2 == 0 or ks > 11 or (ks - 1) * max(ds) > MAX_SPAN:
                raise NotImplementedError(f"resblock kernel_size={ks} dilations={list(ds)}: odd k <= 11 with (k-1)*d <= "
                                          f"{MAX_SPAN} only")
        if len(source_resblock_kernel_sizes) != 2 or len(source_resblock_dilation_sizes) != 2:
            raise NotImplementedError("source_resblock_kernel_sizes: one per upsampling stage (2)")
        if f0_predictor is None:
            f0_predictor = ConvRNNF0Predictor(in_channels=in_channels)
        if not isinstance(f0_predictor, ConvRNNF0Predictor):
            raise NotImplementedError(f"f0_predictor={type(f0_predictor).__name__}: only ConvRNNF0Predictor is built")
        self.in_channels, self.base_channels, self.nb_harmonics = in_channels, base_channels, nb_harmonics
        self.sampling_rate, self.voiced_threshold = sampling_rate, float(nsf_voiced_threshold)
        self.lrelu_slope, self.audio_limit, self.dtype = lrelu_slope, audio_limit, dtype
        self.num_kernels, self.num_upsamples = len(resblock_kernel_sizes), 2
        self.upsample_scale = 8 * 8 * 4
        self.m_source = _Source(nb_harmonics + 1)
        self.conv_pre = weight_norm(nn.Conv1d(in_channels, base_channels, 7, 1, padding=3))
        self.ups = nn.ModuleList(weight_norm(nn.ConvTranspose1d(base_channels // 2 ** i, base_channels // 2 ** (i + 1), 16, 8,
                                                                padding=4)) for i in range(2))
        self.source_downs = nn.ModuleList([nn.Conv1d(18, base_channels // 2, 16, 8, padding=4),
                                           nn.Conv1d(18, base_channels // 4, 1, 1)])
        self.source_resblocks = nn.ModuleList(ResBlock(base_channels // 2 ** (i + 1), k, d) for i, (k, d) in
                                              enumerate(zip(source_resblock_kernel_sizes, source_resblock_dilation_sizes)))
        self.resblocks = nn.ModuleList(ResBlock(base_channels // 2 ** (i + 1), k, d) for i in range(2)
                                       for k, d in zip(resblock_kernel_sizes, resblock_dilation_sizes))
        self.conv_post = weight_norm(nn.Conv1d(base_channels // 4, 18, 7, 1, padding=3))
        self.f0_predictor = f0_predictor
        self._packs: Dict[torch.dtype, PackedHiFT] = {}

    # ---- weights
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        self._packs.clear()
        return super().load_state_dict(_legacy_keys(state_dict), strict=strict, **kw)

    def _apply(self, fn, *a, **kw):
        self._packs.clear()
        return super()._apply(fn, *a, **kw)

    def packed(self, dtype: Optional[torch.dtype] = None) -> PackedHiFT:
        """the weights folded and packed for `dtype` (fp32 | bf16), built once; call load_state_dict / .to() to rebuild."""
        dtype = self.dtype if dtype is None else dtype
        if dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"weight dtype {dtype}: fp32 or bf16")
        if dtype not in self._packs:
            with torch.no_grad():
                self._packs[dtype] = PackedHiFT(self, dtype)
        return self._packs[dtype]

    # ---- stages (channel-last rows)
    def _rows(self, speech_feat: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
        if speech_feat.dim() != 3 or speech_feat.shape[1] != self.in_channels:
            raise ValueError(f"speech_feat must be [B, {self.in_channels}, T], got {tuple(speech_feat.shape)}")
        ptr(speech_feat)                                     # raises on a CPU tensor: no eager fallback
        B, C, T = speech_feat.shape
        x = torch.zeros((B * T, -(-C // 64) * 64), dtype=torch.float32, device=speech_feat.device)
        x[:, :C] = speech_feat.float().transpose(1, 2).reshape(B * T, C)
        return x, B, T

    @torch.no_grad()
    def predict_f0(self, speech_feat: torch.Tensor, dtype=None) -> torch.Tensor:
        """mel [B, 80, T] -> f0 [B, T] (Hz)."""
        pk = self.packed(dtype)
        x, B, T = self._rows(speech_feat)
        for c in pk.f0_convs:
            x = hift_conv(x, c, B, T, elu=True)
        return conv_small(x, pk.f0_cls_w, pk.f0_cls_b, B, T, T, absval=True).reshape(B, T)

    def make_draws(self, B: int, L: int, seed: Optional[int], device) -> Tuple[torch.Tensor, torch.Tensor]:
        g = torch.Generator(device=device)
        if seed is None:
            g.seed()
        else:
            g.manual_seed(int(seed))
        H = self.nb_harmonics + 1
        phase = (torch.rand((B, H, 1), generator=g, device=device) * 2 - 1) * math.pi
        return phase, torch.randn((B, H, L), generator=g, device=device)

    @torch.no_grad()
    def source(self, f0: torch.Tensor, draws=None, seed: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """f0 [B, T] -> (source s [B, T*256], uv [B, T*256]); draws = (phase [B, 9, 1], noise [B, 9, T*256])."""
        pk = self.packed(torch.float32)
        ptr(f0)
        B, T = f0.shape
        H, rep = self.nb_harmonics + 1, self.upsample_scale
        L = T * rep
        phase, noise = draws if draws is not None else self.make_draws(B, L, seed, f0.device)
        phase = phase.to(f0.device, torch.float32).reshape(B, H).clone()
        phase[:, 0] = 0
        noise = noise.to(f0.device, torch.float32).reshape(B, H, L).contiguous()
        f0 = f0.float().contiguous()
        harm = torch.arange(1, H + 1, device=f0.device, dtype=torch.float32).reshape(1, H, 1)
        inc = (f0.reshape(B, 1, T) * harm).reshape(B * H, T).contiguous()
        cum = scan(inc, L, rep, div=float(self.sampling_rate))
        s = torch.empty((B, L), dtype=torch.float32, device=f0.device)
        uv = torch.empty_like(s)
        check(lib().cvft_hift_source(B, H, L, rep, ptr(f0), ptr(cum), ptr(phase), ptr(noise), ptr(pk.lw), ptr(pk.lb),
                                     self.voiced_threshold, ptr(s), ptr(uv), stream()), "cvft_hift_source")
        return s, uv

    @torch.no_grad()
    def decode(self, speech_feat: torch.Tensor, s: torch.Tensor, dtype=None, taps: Optional[dict] = None) -> torch.Tensor:
        """mel [B, 80, T] + source s [B, 1, T*256] -> wav [B, T*256].  taps: a dict that receives the intermediates
        (channel-last rows): conv_pre, stage0, stage1, conv_post."""
        pk = self.packed(dtype)
        x, B, T = self._rows(speech_feat)
        L = T * self.upsample_scale
        s = s.to(torch.float32).reshape(B, L).contiguous()
        s_stft = stft(s)                                             # [B*(64T+1), 18]
        F = L // 4 + 1
        x = hift_conv(x, pk.conv_pre, B, T)
        if taps is not None:
            taps["conv_pre"] = x
        Tin = T
        for i in range(2):
            last = i == 1
            Tout = Tin * 8 + (1 if last else 0)
            C = pk.ups[i][0].Cout
            xu = torch.empty((B * Tout, C), dtype=torch.float32, device=x.device)
            for ph, p in enumerate(pk.ups[i]):
                hift_conv(x, p, B, Tin, pre=PRE_LEAKY, slope=self.lrelu_slope, out=xu, Tq=Tin, Tout=Tout, out_stride=8,
                          out_off=ph + (1 if last else 0))
            if last:                                                  # ReflectionPad1d((1, 0)): row 0 = unpadded row 1
                v = xu.view(B, Tout, C)
                v[:, 0] = v[:, 2]
            if last:
                si = conv_small(s_stft, pk.down_w[i], pk.down_b[i], B, F, Tout)
            else:
                si = conv_small(s_stft, pk.down_w[i], pk.down_b[i], B, F, Tout, stride=8, pad=4)
            x = pk.src_rb[i].run(si, B, Tout, res2=xu)               # x = ups(x) + source_resblocks(source_downs(s_stft))
            xs = torch.empty_like(x)
            nk = self.num_kernels
            for j in range(nk):
                pk.rbs[i * nk + j].run(x, B, Tout, out=xs, accum=j > 0, scale=1.0 / nk if j == nk - 1 else 1.0)
            x, Tin = xs, Tout
            if taps is not None:
                taps[f"stage{i}"] = x
        x = hift_conv(x, pk.conv_post, B, Tin, pre=PRE_LEAKY, slope=0.01)
        if taps is not None:
            taps["conv_post"] = x
        return istft(x, B, self.audio_limit)

    @torch.no_grad()
    def inference(self, speech_feat: torch.Tensor, cache_source: Optional[torch.Tensor] = None, draws=None,
                  seed: Optional[int] = None, dtype=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """speech_feat [B, 80, T] -> (wav [B, T*256], source [B, 1, T*256]); the first cache_source.shape[2] samples of
        the source are overwritten with cache_source before decoding.  draws / seed pin the source's random phase and
        noise."""
        f0 = self.predict_f0(speech_feat, dtype)
        s, _ = self.source(f0, draws, seed)
        s = s.unsqueeze(1)
        if cache_source is not None and cache_source.shape[2] != 0:
            s[:, :, :cache_source.shape[2]] = cache_source.to(s.device, s.dtype)
        return self.decode(speech_feat, s, dtype), s

    def forward(self, *a, **kw):
        raise NotImplementedError("HiFTGenerator is inference only: call .inference()")


def conv_flops(m: HiFTGenerator, T: int) -> int:
    """algorithmic FLOPs (2 per multiply-add) of one utterance of T mel frames, from the module's own shapes."""
    def c(conv, rows):
        w = conv.parametrizations.weight.original1 if hasattr(conv, "parametrizations") else conv.weight
        return 2 * rows * w.numel()
    total = sum(c(m.f0_predictor.condnet[2 * i], T) for i in range(5)) + c(m.conv_pre, T)
    rows = T
    for i in range(2):
        total += c(m.ups[i], rows)                  # every input row meets every weight once
        rows = rows * 8 + (1 if i == 1 else 0)
        total += c(m.source_downs[i], rows)
        for rb in [m.source_resblocks[i]] + list(m.resblocks[i * m.num_kernels:(i + 1) * m.num_kernels]):
            total += sum(c(cv, rows) for cv in list(rb.convs1) + list(rb.convs2))
    return total + c(m.conv_post, rows)
