#!/usr/bin/env python3
"""Golden vectors for streaming synthesis (tests/golden/stream_*.npz, stream_meta.json).

Runs the REFERENCE's own ``CosyVoiceModel(llm=None, flow, hift).tts(source_speech_token=..., stream=True)`` on the CPU: the
tiny Flow of the existing fixtures (tools/make_golden.py) and the shaped HiFT weights of tests/hift_fixtures.py, with
``token_min_hop_len = token_max_hop_len = 30`` set on the instance.  The Flow is called through a recording wrapper that
normalises the prompt mel and de-normalises the result (MEL_MEAN / MEL_STD), which is how the reference's inference
script runs it.  ``cosyvoice.cli.model`` imports
modules that are not needed here (``torchaudio``): empty stand-ins go into ``sys.modules`` first.

Per chunk it records the token window (stream_meta.json), the vocoder's speech (every 16th sample) and the emitted chunk
in stream_<case>.npz, the Flow's output, the vocoder's input mel, the new overlap and the cached mel in
stream_<case>_mel.npz, and the vocoder's source in full in stream_<case>_src.npz (three files, so that each stays below
the largest hift_*.npz).  The random draws are not stored: they are re-drawn
from the case's seed (``stream_fixtures.redraw``), which the tool checks against what the reference drew.

A case is refused when any chunk's speech reaches the +-0.99 clamp or when it has fewer streamed (non-final) chunks than
the case states: 3 for the 130-token case; the 100-token case has 2 by the reference's own schedule (0-50, 30-80, then
the final 60-100).

usage: python tools/make_golden_stream.py
"""
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import make_golden as MG  # noqa: E402  (puts the reference on sys.path and the torchaudio / omegaconf stand-ins in)
from hift_fixtures import shaped_weights  # noqa: E402
from stream_fixtures import CASES, HOP, OVERLAP, SPEECH_STRIDE, make_inputs, redraw  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
MIN_STREAMED = {"noprompt": 3, "prompt": 2}
LIMIT = os.path.getsize(os.path.join(GOLD, "hift_t137.npz"))


def main():
    for name in ("onnxruntime", "tensorrt", "hyperpyyaml", "whisper"):
        sys.modules.setdefault(name, types.ModuleType(name))
    from cosyvoice.cli.model import BOUNDARY_TRIM_RATIO, CosyVoiceModel
    from cosyvoice.hifigan.f0_predictor import ConvRNNF0Predictor
    from cosyvoice.hifigan.generator import HiFTGenerator
    from torch.distributions.uniform import Uniform
    from cosyvoice_lora_finetune_framework_amd.config import INFERENCE_CONFIG, MEL_MEAN, MEL_STD
    assert BOUNDARY_TRIM_RATIO == INFERENCE_CONFIG["boundary_trim_ratio"]

    torch.manual_seed(0)
    flow = MG.build_ref_flow('vendored', **MG.TINY_FLOW)
    MG.wrap_and_fill(flow, r=4, alpha=8, targets=MG.FLOW_TARGETS, seed=3)
    flow.eval()
    hift = HiFTGenerator(f0_predictor=ConvRNNF0Predictor()).eval()
    w = np.load(os.path.join(GOLD, "hift_weights.npz"))
    spec = [(k, tuple(v.shape)) for k, v in hift.state_dict().items()]
    hift.load_state_dict(shaped_weights(spec, (w["classifier_weight"], w["classifier_bias"])), strict=True)

    rec = {}
    flow_inference, hift_inference = flow.inference, hift.inference

    def flow_in_log_mel(**kw):
        """what token2wav calls as flow.inference: the Flow works on normalised mels, the caller on log-mels; the
        de-normalised output is recorded"""
        feat = kw["prompt_feat"]
        kw["prompt_feat"] = (feat - MEL_MEAN) / MEL_STD if feat.shape[1] > 0 else feat
        with torch.inference_mode():
            mel, cache = flow_inference(**kw)
            mel = mel * MEL_STD + MEL_MEAN
        rec["flow_mel"] = mel.clone()
        return mel, cache

    def rec_hift_inference(speech_feat, cache_source=torch.zeros(1, 1, 0)):
        with torch.no_grad():
            speech, source = hift_inference(speech_feat=speech_feat, cache_source=cache_source)
        rec.update(mel=speech_feat.clone(), speech=speech.clone(), source=source.clone())
        return speech, source

    flow.inference, hift.inference = flow_in_log_mel, rec_hift_inference
    model = CosyVoiceModel(None, flow, hift)
    model.token_min_hop_len = model.token_max_hop_len = HOP
    assert model.token_overlap_len == OVERLAP and model.mel_overlap_len == 34 and model.source_cache_len == 5120

    meta = dict(hop=HOP, overlap=OVERLAP, boundary_trim_ratio=BOUNDARY_TRIM_RATIO, speech_stride=SPEECH_STRIDE, cases={})
    for name, c in CASES.items():
        tokens, ptok, pfeat, emb = make_inputs(c)
        drawn, arr, mels, src, windows, per_chunk = [], {}, {}, {}, [], []
        u_sample, randn_like = Uniform.sample, torch.randn_like

        def rec_sample(self, sample_shape=torch.Size()):
            v = u_sample(self, sample_shape)
            drawn.append(("uniform", v.clone()))
            return v

        def rec_randn_like(x, *a, **kw):
            v = randn_like(x, *a, **kw)
            drawn.append(("randn", v.clone()))
            return v
        Uniform.sample, torch.randn_like = rec_sample, rec_randn_like
        try:
            torch.manual_seed(c["seed"])
            consumed, peak = 0, 0.0
            for i, item in enumerate(model.tts(flow_embedding=emb, flow_prompt_speech_token=ptok, prompt_speech_feat=pfeat,
                                               source_speech_token=tokens, stream=True)):
                (uuid,) = list(model.hift_cache_dict.keys())
                final = rec["mel"].shape[2] * 256 == item["tts_speech"].shape[1]
                stop = c["n_tokens"] if final else consumed + HOP + OVERLAP
                windows.append((consumed, stop, bool(final)))
                assert int(rec["flow_mel"].shape[2]) == int((stop - consumed) / 50 * 22050 / 256), "token window"
                consumed += HOP
                p = f"c{i}_"
                mels[p + "flow_mel"], mels[p + "mel"] = rec["flow_mel"][0], rec["mel"][0]
                arr[p + "speech"] = rec["speech"][0, ::SPEECH_STRIDE]
                arr[p + "out"] = item["tts_speech"][0]
                src[p + "source"] = rec["source"][0, 0]
                if not final:
                    mels[p + "overlap"] = model.mel_overlap_dict[uuid][0].clone()
                    mels[p + "cache_mel"] = model.hift_cache_dict[uuid]["mel"][0].clone()
                    assert torch.equal(model.hift_cache_dict[uuid]["source"][0, 0], rec["source"][0, 0, -5120:])
                peak = max(peak, float(rec["speech"].abs().max()))
                assert float(rec["speech"].abs().max()) < 0.99, f"{name}: chunk {i} reaches the clamp"
                per_chunk.append(len(drawn) - sum(per_chunk))
        finally:
            Uniform.sample, torch.randn_like = u_sample, randn_like
        assert [tuple(x) for x in windows] == [tuple(x) for x in c["windows"]], (windows, c["windows"])
        streamed = sum(1 for x in windows if not x[2])
        assert streamed >= MIN_STREAMED[name], f"{name}: only {streamed} streamed chunks"
        plan = [(k, list(v.shape)) for k, v in drawn]
        again = redraw(c["seed"], plan)
        assert all(torch.equal(a, b[1]) for a, b in zip(again, drawn)), "the draws cannot be redrawn"
        assert all(n == 4 for n in per_chunk) and [k for k, _ in plan[:4]] == ["randn", "uniform", "randn", "randn"], plan[:4]
        trim = int(c["prompt_frames"] * BOUNDARY_TRIM_RATIO)
        for path, data in ((f"stream_{name}.npz", arr), (f"stream_{name}_mel.npz", mels), (f"stream_{name}_src.npz", src)):
            path = os.path.join(GOLD, path)
            np.savez_compressed(path, **{k: v.numpy() for k, v in data.items()})
            assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path), LIMIT)
            print(path, os.path.getsize(path), "bytes")
        meta["cases"][name] = dict(n_tokens=c["n_tokens"], prompt_frames=c["prompt_frames"], prompt_tokens=c["prompt_tokens"],
                                   seed=c["seed"], input_seed=c["input_seed"], windows=windows, trim=trim, draw_plan=plan,
                                   draws_per_chunk=per_chunk, peak=peak)
        print(name, windows, "trim", trim, "peak", peak)
    with open(os.path.join(GOLD, "stream_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
