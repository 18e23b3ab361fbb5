"""The HiFT vocoder on the GPU: the csrc/hift.hip kernels against torch on the CPU, and HiFTGenerator stage by stage and
end to end against the reference's own outputs (tests/golden/hift_*.npz, tools/make_golden_hift.py)."""
import json
import math
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4            # the project's fp32 parity bound: max abs error / max abs reference value
CASES = ["t40", "t137", "b2"]


def H():
    from cosyvoice_lora_finetune_framework_amd import hift
    return hift


def err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max())


def _meta():
    return json.load(open(os.path.join(GOLD, "hift_meta.json")))


def _state_dict(m):
    from hift_fixtures import shaped_weights
    w = np.load(os.path.join(GOLD, "hift_weights.npz"))
    spec = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    return shaped_weights(spec, (w["classifier_weight"], w["classifier_bias"]))


_MODEL = {}


def model():
    if "m" not in _MODEL:
        m = H().HiFTGenerator()
        m.load_state_dict(_state_dict(m), strict=True)
        _MODEL["m"] = m.to(DEV).eval()
    return _MODEL["m"]


def case(name):
    from hift_fixtures import make_mel, redraw
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, f"hift_{name}.npz")).items()}
    c = _meta()["cases"][name]
    phase, noise = redraw(c["seed"], c["B"], c["T"] * 256)
    g["mel"] = make_mel(c["T"], c["mel_seed"]).repeat(c["B"], 1, 1)
    g["uv"] = (g["f0"] > 10).repeat_interleave(256, dim=1).to(torch.uint8)        # the reference's uv = f0 > 10, per sample
    return g, c, (phase.to(DEV), noise.to(DEV))


# ------------------------------------------------------------------------------------------------ ops
def _conv_ref(x, w, bias, taps, pre, alpha, slope, wdtype):
    """fp64 restatement of cvft_hift_conv's product on the operands as the kernel rounds them.  x [B, T, Cin],
    w [ntaps, Cout, Cin]."""
    x = x.double()
    if pre == 1:
        x = x.float()
        a = alpha.float()
        x = (x + (1.0 / (a + 1e-9)) * torch.sin(x * a) ** 2).double()
    elif pre == 2:
        x = torch.where(x > 0, x, x * float(np.float32(slope)))
    x = x.float().to(wdtype).double()
    w = w.to(wdtype).double()
    B, T, _ = x.shape
    lo, hi = min(taps), max(taps)
    xp = F.pad(x, (0, 0, max(0, -lo), max(0, hi)))
    y = torch.zeros(B, T, w.shape[1], dtype=torch.float64)
    for j, o in enumerate(taps):
        y += xp[:, o + max(0, -lo): o + max(0, -lo) + T] @ w[j].t()
    return y + (bias.double() if bias is not None else 0.0)


# (k, d, pre, epilogue, Cin, Cout): every form the model launches
CONV_FORMS = [(k, d, 1, e, 128, 128) for k in (3, 7, 11) for d, e in ((1, "res"), (3, "none"), (5, "none"))] + \
             [(3, 1, 1, "res_accum_scale", 256, 256), (7, 1, 1, "res_res2", 128, 128), (11, 1, 1, "res_accum_scale", 128, 128),
              (7, 1, 0, "none", 80, 512), (7, 1, 2, "none", 128, 18), (3, 1, 0, "elu", 80, 512), (3, 1, 0, "elu", 512, 512)]


@pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T", [77, 9])
@pytest.mark.parametrize("k, d, pre, epi, Cin, Cout", CONV_FORMS)
def test_conv_kernel_forms(k, d, pre, epi, Cin, Cout, T, wdtype):
    """T = 77 is not a multiple of the 64-row tile, T = 9 is smaller than the halo of every dilated form.  The
    reference is an fp64 product of the operands rounded to the weight dtype, so only the fp32 accumulation differs."""
    h = H()
    B = 2
    g = torch.Generator().manual_seed(k * 100 + d * 10 + T)
    CinP = -(-Cin // 64) * 64
    x = torch.zeros(B, T, CinP)
    x[..., :Cin] = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)
    bias = torch.randn(Cout, generator=g) * 0.1
    alpha = 1.0 + 0.3 * torch.randn(CinP, generator=g)
    res, res2, old = (torch.randn(B, T, Cout, generator=g) for _ in range(3))
    pk = h.pack_conv1d(w.to(DEV), bias.to(DEV), d, wdtype)
    slope = 0.01
    want = _conv_ref(x[..., :Cin], w.permute(2, 0, 1), bias, pk.offsets, pre, alpha[:Cin], slope, wdtype)
    kw = {}
    if epi == "elu":
        want = torch.where(want > 0, want, torch.expm1(want))
        kw = dict(elu=True)
    if epi.startswith("res"):
        want = want + res.double()
        kw = dict(res=res.reshape(B * T, Cout).to(DEV))
    if epi == "res_res2":
        want = want + res2.double()
        kw["res2"] = res2.reshape(B * T, Cout).to(DEV)
    out = None
    if epi == "res_accum_scale":
        want = (want + old.double()) * float(np.float32(1.0 / 3))
        out = old.reshape(B * T, Cout).clone().to(DEV)
        kw.update(accum=True, scale=1.0 / 3, out=out)
    got = h.hift_conv(x.reshape(B * T, CinP).to(DEV), pk, B, T, pre=pre, alpha=alpha.to(DEV) if pre == 1 else None,
                      slope=slope, **kw)
    e = err(got.reshape(B, T, Cout), want)
    print(f"conv k={k} d={d} pre={pre} {epi} {Cin}->{Cout} T={T} {wdtype}: {e:.3g}")
    assert e <= TOL


@pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T, last", [(21, False), (5, True)])
def test_transposed_conv_phases(T, last, wdtype):
    """ConvTranspose1d(k 16, s 8, p 4) as 8 phase launches with the leaky-ReLU staged, against F.conv_transpose1d;
    `last` writes at row offset 1 of 8T + 1 rows (the reflection-padded stage)."""
    h = H()
    B, Cin, Cout = 2, 128, 64
    g = torch.Generator().manual_seed(5 + T)
    x = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(Cin, Cout, 16, generator=g) / math.sqrt(Cin * 2)
    bias = torch.randn(Cout, generator=g) * 0.1
    xr = F.leaky_relu(x, 0.1).to(wdtype).double()
    want = F.conv_transpose1d(xr.transpose(1, 2), w.to(wdtype).double(), bias.double(), stride=8, padding=4).transpose(1, 2)
    Tout = 8 * T + int(last)
    out = torch.zeros(B * Tout, Cout, device=DEV)
    for ph, p in enumerate(h.pack_conv_transpose_k16s8(w.to(DEV), bias.to(DEV), wdtype)):
        h.hift_conv(x.reshape(B * T, Cin).to(DEV), p, B, T, pre=h.PRE_LEAKY, slope=0.1, out=out, Tq=T, Tout=Tout,
                    out_stride=8, out_off=ph + int(last))
    got = out.reshape(B, Tout, Cout)[:, int(last):]
    assert err(got, want) <= TOL
    if last:
        assert float(out.reshape(B, Tout, Cout)[:, 0].abs().max()) == 0.0


def test_conv_small_against_torch():
    h = H()
    g = torch.Generator().manual_seed(9)
    B, Tin = 2, 129
    x = torch.randn(B, Tin, 18, generator=g)
    for (Cout, k, s, p) in ((256, 16, 8, 4), (128, 1, 1, 0)):
        w = torch.randn(Cout, 18, k, generator=g) * 0.1
        b = torch.randn(Cout, generator=g)
        want = F.conv1d(x.double().transpose(1, 2), w.double(), b.double(), stride=s, padding=p).transpose(1, 2)
        Tout = want.shape[1]
        got = h.conv_small(x.reshape(B * Tin, 18).to(DEV), w.permute(2, 1, 0).contiguous().to(DEV), b.to(DEV), B, Tin, Tout,
                           stride=s, pad=p)
        assert err(got.reshape(B, Tout, Cout), want) <= TOL
    w = torch.randn(1, 18, 1, generator=g)
    got = h.conv_small(x.reshape(B * Tin, 18).to(DEV), w.permute(2, 1, 0).contiguous().to(DEV), None, B, Tin, Tin, absval=True)
    assert err(got.reshape(B, Tin), (x.double() @ w[0, :, 0].double()).abs()) <= TOL


def test_stft_istft_against_torch():
    h = H()
    g = torch.Generator().manual_seed(4)
    B, L = 2, 4 * 333
    s = torch.randn(B, L, generator=g)
    win = torch.hann_window(16, periodic=True, dtype=torch.float64)
    spec = torch.stft(s.double(), 16, 4, 16, window=win, return_complex=True)                 # [B, 9, F]
    want = torch.cat([spec.real, spec.imag], 1).transpose(1, 2)                              # [B, F, 18]
    got = h.stft(s.to(DEV)).reshape(B, L // 4 + 1, 18)
    assert err(got, want) <= TOL
    Fr = L // 4 + 1
    x = torch.randn(B, Fr, 18, generator=g)
    mag, ph = torch.exp(x[..., :9].double()).clamp(max=1e2), torch.sin(x[..., 9:].double())
    z = torch.complex(mag * torch.cos(ph), mag * torch.sin(ph)).transpose(1, 2)
    want = torch.istft(z, 16, 4, 16, window=win).clamp(-0.99, 0.99)
    got = h.istft(x.reshape(B * Fr, 18).to(DEV), B)
    assert got.shape == want.shape and err(got, want) <= TOL


def test_scan_accumulates_in_fp64():
    """at 256 000 samples an fp32 running sum is off by ~1e-3; the kernel's is the fp64 sum rounded to fp32 (an
    element may differ by one rounding where the partial sums associate differently)."""
    h = H()
    g = torch.Generator().manual_seed(6)
    L = 256000
    x = torch.rand(3, L, generator=g) * 0.1
    want = torch.cumsum(x.double(), 1)
    got = h.scan(x.to(DEV), L).cpu()
    assert float(((got.double() - want).abs() / want).max()) <= 2.0 ** -23
    assert int((got != want.float()).sum()) <= 3
    xr = torch.rand(3, 1000, generator=g) * 0.1
    got = h.scan(xr.to(DEV), L, rep=256).cpu()
    want = torch.cumsum(xr.double().repeat_interleave(256, dim=1), 1)
    assert float(((got.double() - want).abs() / want).max()) <= 2.0 ** -23


def test_istft_clip_and_clamp_case():
    """conv_post-like input that reaches the 1e2 magnitude clip and the +-0.99 clamp, against the reference's ISTFT."""
    h = H()
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "hift_clip.npz")).items()}
    wav, mag = h.istft(g["x"].to(DEV), 1, want_mag=True)
    assert float((g["mag"] == 100).float().mean()) >= 0.01 and float((g["wav"].abs() == np.float32(0.99)).float().mean()) >= 0.01
    assert err(wav, g["wav"]) <= TOL and err(mag, g["mag"]) <= TOL
    assert torch.equal(mag.cpu() == 100, g["mag"] == 100)
    assert torch.equal(wav.cpu().abs() == np.float32(0.99), g["wav"].abs() == np.float32(0.99))


# ------------------------------------------------------------------------------------------------ stages (fp32)
@pytest.mark.parametrize("name", CASES)
def test_f0_stage(name):
    g, c, _ = case(name)
    f0 = model().predict_f0(g["mel"].to(DEV))
    e = err(f0, g["f0"])
    print(f"{name}: f0 {e:.3g}")
    assert e <= TOL


@pytest.mark.parametrize("name", CASES)
def test_source_stage(name):
    """the fixture's f0 and the reference's draws -> source; uv exactly."""
    g, c, draws = case(name)
    s, uv = model().source(g["f0"].to(DEV), draws)
    assert torch.equal(uv.cpu().to(torch.uint8), g["uv"])
    e = err(s.unsqueeze(1), g["s"])
    print(f"{name}: source {e:.3g}")
    assert e <= TOL


@pytest.mark.parametrize("name", CASES)
def test_decode_stages(name):
    """mel + the fixture's source -> every stored intermediate (sub-sampled rows) and the wav."""
    g, c, _ = case(name)
    taps = {}
    m = model()
    # through inference(): a full-length cache_source replaces the device's own source with the fixture's
    wav, s = m.inference(g["mel"].to(DEV), cache_source=g["s"].to(DEV), seed=0)
    assert torch.equal(s.cpu(), g["s"])
    wav2 = m.decode(g["mel"].to(DEV), g["s"].to(DEV), taps=taps)
    assert torch.equal(wav, wav2)
    for key in ("conv_pre", "stage0", "stage1", "conv_post"):
        e = err(taps[key][g[key + "_rows"].long().to(DEV)], g[key])
        print(f"{name}: {key} {e:.3g}")
        assert e <= TOL, key
    e = err(wav, g["wav"])
    print(f"{name}: wav {e:.3g}")
    assert e <= TOL


E2E_SOURCE_BOUND = 9.3e-3        # 2 x 4.63e-3
E2E_WAV_BOUND = 4.5e-3           # 2 x 2.23e-3


@pytest.mark.parametrize("name", CASES)
def test_end_to_end_from_the_mel(name):
    """Only the draws are fed in; the device's own f0 drives the source.  NOT held to 1e-4: the phase is a running sum
    of f0 * h / sr, so a relative f0 error e grows to about e * f0 * h / sr * 256 * sqrt(frames) cycles at the end of the
    utterance (h = 9, f0 = 250 Hz, 137 frames, e = 1e-6: ~3e-4 cycles = 2e-3 rad), and the fp32 rounding of the sum
    (one ulp is 2.4e-4 cycles beyond 2048 cycles) can land on the other side for a sample; the reference is that sensitive
    to its own f0.  uv must still be exactly the reference's (the fixtures keep every frame's f0 0.5 Hz away from the
    threshold).  Bound: twice the worst measured value, never looser than 2e-2 of peak.
    Measured (MI355X, fp32; source / wav, of peak): T = 40 7.9e-4 / 5.6e-4, T = 137 4.63e-3 / 2.23e-3, B = 2 1.08e-3 / 7.95e-4."""
    g, c, draws = case(name)
    m = model()
    f0 = m.predict_f0(g["mel"].to(DEV))
    _, uv = m.source(f0, draws)
    assert torch.equal(uv.cpu().to(torch.uint8), g["uv"])
    wav, s = m.inference(g["mel"].to(DEV), draws=draws)
    es, ew = err(s, g["s"]), err(wav, g["wav"])
    print(f"{name}: end to end source {es:.3g} wav {ew:.3g}")
    assert es <= E2E_SOURCE_BOUND and ew <= E2E_WAV_BOUND


def test_partial_cache_source_overwrites_its_prefix():
    g, c, draws = case("t40")
    m = model()
    _, s0 = m.inference(g["mel"].to(DEV), draws=draws)
    n = 1000
    cache = torch.full((1, 1, n), 0.123, device=DEV)
    _, s1 = m.inference(g["mel"].to(DEV), cache_source=cache, draws=draws)
    assert torch.equal(s1[:, :, :n], cache) and torch.equal(s1[:, :, n:], s0[:, :, n:])


def test_fp32_is_deterministic_and_rows_are_independent():
    g, c, draws = case("b2")
    m = model()
    mel = g["mel"].to(DEV)
    w1, s1 = m.inference(mel, draws=draws)
    w2, s2 = m.inference(mel, draws=draws)
    assert torch.equal(w1, w2) and torch.equal(s1, s2)
    for b in range(2):
        wb, sb = m.inference(mel[b:b + 1], draws=(draws[0][b:b + 1], draws[1][b:b + 1]))
        assert torch.equal(wb[0], w1[b]) and torch.equal(sb[0], s1[b])


def test_seeded_draws():
    g, c, _ = case("t40")
    m = model()
    a, _ = m.inference(g["mel"].to(DEV), seed=3)
    b, _ = m.inference(g["mel"].to(DEV), seed=3)
    d, _ = m.inference(g["mel"].to(DEV), seed=4)
    assert torch.equal(a, b) and not torch.equal(a, d)


# ------------------------------------------------------------------------------------------------ bf16
BF16_WAV_BOUND = 3.4e-2          # 2 x 1.70e-2
BF16_POST_BOUND = 3.7e-2         # 2 x 1.87e-2


@pytest.mark.parametrize("name", CASES)
def test_bf16_path_against_the_reference(name):
    """bf16 weights and staged operands, fp32 accumulation and activations, fed the fixture's source so that only the
    filter network's arithmetic is compared.  exp() of the conv_post output amplifies the rounding.  Bound: twice the
    worst measured value, never looser than 5e-2 of peak for the wav.  Measured (MI355X), T = 40 / T = 137 / B = 2:
    conv_post (stored rows) 1.30e-2 / 1.35e-2 / 1.87e-2, wav 1.54e-2 / 1.39e-2 / 1.70e-2 of peak."""
    g, c, _ = case(name)
    taps = {}
    wav = model().decode(g["mel"].to(DEV), g["s"].to(DEV), dtype=torch.bfloat16, taps=taps)
    ep = err(taps["conv_post"][g["conv_post_rows"].long().to(DEV)], g["conv_post"])
    ew = err(wav, g["wav"])
    print(f"{name}: bf16 conv_post {ep:.3g} wav {ew:.3g}")
    assert ew <= BF16_WAV_BOUND and ep <= BF16_POST_BOUND


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_writes_the_vocoded_wav(tmp_path, monkeypatch):
    """inference_joint.main with --hift / --wav on tiny merged LLM / Flow files: the wav's samples are vocode() of the
    CLI's mel to 16-bit rounding; without --hift the mel file is the same and no wav appears."""
    from helpers import build_flow_product, build_llm_product
    from cosyvoice_lora_finetune_framework_amd import utils as U
    from cosyvoice_lora_finetune_framework_amd.inference_joint import main, pcm16, vocode
    from cosyvoice_lora_finetune_framework_amd.lora import get_merged_state_dict
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    arr = dict(np.load(os.path.join(GOLD, "llm_decode_tiny.npz")))
    ref = dict(np.load(os.path.join(GOLD, "llm_decode_joint.npz")))
    meta = json.load(open(os.path.join(GOLD, "tiny_meta.json")))
    dmeta = json.load(open(os.path.join(GOLD, "llm_decode_meta.json")))
    llm = build_llm_product(dmeta["tiny"], DEV, Numerics())
    flow = build_flow_product(meta["flow"], DEV, Numerics())
    torch.save({k: v.cpu() for k, v in get_merged_state_dict(llm).items()}, tmp_path / "llm.pt")
    torch.save({k: v.cpu() for k, v in get_merged_state_dict(flow).items()}, tmp_path / "flow.pt")
    torch.save({k: v.cpu() for k, v in model().state_dict().items()}, tmp_path / "hift.pt")
    np.save(tmp_path / "z.npy", ref["z"])
    c = dmeta["tiny"]["build"]
    llm_cfg = dict(text_encoder_input_size=c["text_in"], llm_input_size=c["d"], llm_output_size=c["d"],
                   text_token_size=c["text_vocab"], speech_token_size=c["speech_vocab"], attention_heads=c["heads"],
                   linear_units=c["ff"], text_encoder_blocks=c["text_blocks"], llm_blocks=c["llm_blocks"])
    common = ["--llm", str(tmp_path / "llm.pt"), "--flow", str(tmp_path / "flow.pt"),
              "--text-tokens", ",".join(str(int(t)) for t in arr["i_text"][0]), "--top-k", "1", "--tau-r", "1e9",
              "--llm-config", json.dumps(llm_cfg), "--flow-config", json.dumps(meta["flow"]["build"]),
              "--noise", str(tmp_path / "z.npy")]
    monkeypatch.chdir(tmp_path)
    main(common + ["--out", str(tmp_path / "mel0.npy")])
    assert not (tmp_path / "out.wav").exists() and sorted(p.name for p in tmp_path.iterdir()) == \
        ["flow.pt", "hift.pt", "llm.pt", "mel0.npy", "z.npy"]
    main(common + ["--out", str(tmp_path / "mel1.npy"), "--hift", str(tmp_path / "hift.pt"), "--wav", str(tmp_path / "o.wav"),
                   "--hift-seed", "5"])
    mel0, mel1 = np.load(tmp_path / "mel0.npy"), np.load(tmp_path / "mel1.npy")
    assert np.array_equal(mel0, mel1)
    with wave.open(str(tmp_path / "o.wav")) as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, 22050)
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    want = vocode(model(), torch.from_numpy(mel1)[None].to(DEV), seed=5)
    assert pcm.shape[0] == mel1.shape[1] * 256
    assert np.array_equal(pcm, pcm16(want[0]))
