#!/usr/bin/env python3
"""Golden vectors for the HiFT vocoder (tests/golden/hift_*.npz, hift_meta.json).

Runs the REFERENCE's own ``HiFTGenerator(f0_predictor=ConvRNNF0Predictor()).inference`` on the CPU.  Weights come from
``oracle.detweights`` by key and shape and are not stored, except the shaping applied on top (``shaped_weights`` in
tests/hift_fixtures.py, which the tests call too): Snake alphas are moved to 1 + det, ``conv_post`` is scaled so that the waveform is neither
tiny nor clamped, and the f0 classifier (513 numbers, stored in hift_weights.npz) is solved so that every fixture mel
gives a voiced / unvoiced contour with a margin around the 10 Hz threshold.  The random draws of the source are
re-drawable from the case's seed (``redraw``); the tool checks that against what the reference actually drew.

A case is only written when: voiced and unvoiced frames are each >= 20 %, every frame has |f0 - 10| >= 0.5, no magnitude
reaches the 1e2 clip, no sample reaches the +-0.99 clamp and peak |wav| >= 0.1.  One extra case (hift_clip) does reach
both on >= 1 % of its elements and covers the ISTFT stage only.

usage: python tools/make_golden_hift.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))
from hift_fixtures import POST_SCALE, WEIGHT_SEED, make_mel, redraw, shaped_weights  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
CASES = {"t40": dict(T=40, B=1, seed=401, mel_seed=11), "t137": dict(T=137, B=1, seed=402, mel_seed=12),
         "b2": dict(T=40, B=2, seed=403, mel_seed=11)}
STRIDES = dict(conv_pre=16, stage0=64, stage1=256, conv_post=32)


def f0_target(T: int) -> torch.Tensor:
    """voiced runs (120 .. 300 Hz, slowly varying) alternating with unvoiced runs (3 Hz), 12 / 8 frames each."""
    t = torch.arange(T, dtype=torch.float64)
    voiced = (t % 20) < 12
    return torch.where(voiced, 210.0 + 90.0 * torch.sin(t * 0.13), torch.full_like(t, 3.0))


def main():
    sys.path.insert(0, os.environ.get("CVFT_REFERENCE", "/root/reference/cosyvoice_flow_finetune"))
    from cosyvoice.hifigan.f0_predictor import ConvRNNF0Predictor
    from cosyvoice.hifigan.generator import HiFTGenerator
    from torch.distributions.uniform import Uniform

    torch.manual_seed(0)
    ref = HiFTGenerator(f0_predictor=ConvRNNF0Predictor()).eval()
    spec = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    ref.load_state_dict(shaped_weights(spec), strict=True)

    # ---- solve the classifier on every fixture mel's condnet features (fp64 least squares, min-norm: 177 rows < 512)
    feats, targets = [], []
    with torch.no_grad():
        for name in ("t40", "t137"):
            c = CASES[name]
            h = ref.f0_predictor.condnet(make_mel(c["T"], c["mel_seed"]))[0].t().double()      # [T, 512]
            feats.append(torch.cat([h, torch.ones(h.shape[0], 1, dtype=torch.float64)], 1))
            targets.append(f0_target(c["T"]))
    sol = torch.linalg.lstsq(torch.cat(feats), torch.cat(targets).unsqueeze(1)).solution[:, 0]
    cls = (sol[:-1].float().reshape(1, -1).numpy(), sol[-1:].float().numpy())
    ref.load_state_dict(shaped_weights(spec, cls), strict=True)
    np.savez(os.path.join(GOLD, "hift_weights.npz"), classifier_weight=cls[0], classifier_bias=cls[1])

    meta = dict(weight_seed=WEIGHT_SEED, post_scale=POST_SCALE, keys=[k for k, _ in spec], strides=STRIDES, cases={})
    for name, c in CASES.items():
        T, B = c["T"], c["B"]
        L = T * 256
        mel = make_mel(T, c["mel_seed"]).repeat(B, 1, 1)
        cap, drawn = {}, []
        rb_out = []
        hooks = [ref.conv_pre.register_forward_hook(lambda m, i, o: cap.__setitem__("conv_pre", o.detach().clone())),
                 ref.conv_post.register_forward_hook(lambda m, i, o: cap.__setitem__("conv_post", o.detach().clone())),
                 ref.f0_predictor.register_forward_hook(lambda m, i, o: cap.__setitem__("f0", o.detach().clone()))]
        hooks += [rb.register_forward_hook(lambda m, i, o: rb_out.append(o.detach().clone())) for rb in ref.resblocks]
        u_sample, randn_like = Uniform.sample, torch.randn_like

        def rec_sample(self, sample_shape=torch.Size()):
            v = u_sample(self, sample_shape)
            drawn.append(v.clone())
            return v

        def rec_randn_like(x, *a, **kw):
            v = randn_like(x, *a, **kw)
            drawn.append(v.clone())
            return v
        Uniform.sample, torch.randn_like = rec_sample, rec_randn_like
        try:
            torch.manual_seed(c["seed"])
            wav, s = ref.inference(mel)
        finally:
            Uniform.sample, torch.randn_like = u_sample, randn_like
            for h in hooks:
                h.remove()
        wav, s = wav.clone(), s.clone()
        phase, noise = redraw(c["seed"], B, L)
        assert len(drawn) == 3 and torch.equal(drawn[0], phase) and torch.equal(drawn[1], noise), "draw order changed"
        f0 = cap["f0"]
        stage = [((rb_out[3 * i] + rb_out[3 * i + 1]) + rb_out[3 * i + 2]) / 3 for i in range(2)]
        uv = (f0 > 10).float()
        vfrac = float(uv.mean())
        mag = torch.exp(cap["conv_post"][:, :9])
        assert 0.2 <= vfrac <= 0.8, f"{name}: voiced fraction {vfrac}"
        assert float((f0 - 10).abs().min()) >= 0.5, f"{name}: f0 within 0.5 of the threshold"
        assert float(mag.max()) < 1e2, f"{name}: magnitude clip reached ({float(mag.max())})"
        assert float(wav.abs().max()) < 0.99 and float(wav.abs().max()) >= 0.1, f"{name}: peak {float(wav.abs().max())}"
        cl = lambda x: x.transpose(1, 2).reshape(-1, x.shape[1])          # noqa: E731  [B, C, T] -> rows [B*T, C]
        arr = dict(f0=f0, s=s, wav=wav)
        for key, x in (("conv_pre", cap["conv_pre"]), ("stage0", stage[0]), ("stage1", stage[1]),
                       ("conv_post", cap["conv_post"])):
            rows = torch.arange(0, x.shape[0] * x.shape[2], STRIDES[key])
            arr[key + "_rows"] = rows.to(torch.int32)
            arr[key] = cl(x)[rows]
        np.savez(os.path.join(GOLD, f"hift_{name}.npz"), **{k: v.numpy() for k, v in arr.items()})
        meta["cases"][name] = dict(T=T, B=B, seed=c["seed"], mel_seed=c["mel_seed"], voiced_fraction=vfrac, f0_min=float(f0.min()),
                                   f0_max=float(f0.max()), mag_max=float(mag.max()), peak=float(wav.abs().max()))
        print(name, meta["cases"][name], "bytes", os.path.getsize(os.path.join(GOLD, f"hift_{name}.npz")))

    # ---- the clip / clamp case: ISTFT stage only
    g = torch.Generator().manual_seed(77)
    F = 64 * 8 + 1
    x = torch.randn(1, 18, F, generator=g)
    x[:, :9] = x[:, :9] * 1.8 + 1.0
    x[:, 9:] = x[:, 9:] * 2.0
    with torch.no_grad():
        mag = torch.exp(x[:, :9])
        wav = torch.clamp(ref._istft(mag, torch.sin(x[:, 9:])), -ref.audio_limit, ref.audio_limit)
    clipped, clamped = float((mag > 1e2).float().mean()), float((wav.abs() >= ref.audio_limit).float().mean())
    assert clipped >= 0.01 and clamped >= 0.01, (clipped, clamped)
    np.savez(os.path.join(GOLD, "hift_clip.npz"), x=x[0].t().contiguous().numpy(), wav=wav.numpy(),
             mag=torch.clip(mag, max=1e2)[0].t().contiguous().numpy())
    meta["clip"] = dict(F=F, clipped_fraction=clipped, clamped_fraction=clamped)
    print("clip", meta["clip"])
    with open(os.path.join(GOLD, "hift_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
