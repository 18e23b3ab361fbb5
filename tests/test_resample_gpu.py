"""cvft_resample on the GPU against the fp64 restatement of the published formula (tests/resample_fixtures.py): parity
for every rate pair and the lengths that straddle a tile, ragged batches, determinism, error paths, and the callers --
prepare_joint_data's shards, synthesize(prompt_rate=...) and inference_joint's --wav-rate."""
import functools
import json
import os
import wave

import numpy as np
import pytest
import torch

import resample_fixtures as RF
from helpers import build_flow_product, build_llm_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def A():
    from cosyvoice_lora_finetune_framework_amd import audio
    return audio


def _lengths(pair):
    o, n = RF.ratio(*pair)[:2]
    edge = A().RESAMPLE_TILE * o // n                  # the input length whose output fills one tile
    return [1, o + 1, 3001, edge - 1, edge + 1, 22050]


@functools.lru_cache(maxsize=None)
def _reference(pair, L):
    """(input fp32, fp64 restatement): computed once, shared, read-only."""
    x = RF.noise(L, 1000 + L % 997)
    y = RF.resample_fp64(x, *pair)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@pytest.mark.parametrize("pair", RF.PAIRS)
def test_parity_with_the_fp64_restatement(pair):
    """max |kernel - fp64 restatement| against (span + 1) 2^-24 max_i sum_k |K[i][k]| max|x|, the worst-case rounding
    of a span-term fp32 FMA chain (<= 3.2e-6 for these pairs); measured on the MI355X: see DESIGN.md section 19."""
    rs = A().Resampler(*pair, DEV)
    worst = 0.0
    for L in _lengths(pair):
        assert L <= max(pair)                           # at most one second of audio
        x, want = _reference(pair, L)
        got, lens = rs(torch.from_numpy(x.copy()).to(DEV))
        M = RF.out_length(L, *pair)
        assert lens == [M] == [A().resampled_length(L, *pair)] and tuple(got.shape) == (1, M)
        tol = RF.tolerance(*pair, x)
        assert tol <= 3.2e-6
        err = float(np.abs(got[0].cpu().numpy().astype(np.float64) - want).max())
        worst = max(worst, err)
        print(f"{pair[0]} -> {pair[1]} L={L}: max |y - fp64| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (pair, L, err, tol)
    print(f"{pair[0]} -> {pair[1]}: worst {worst:.3e}")


@pytest.mark.parametrize("pair", [(48000, 22050), (22050, 48000), (16000, 22050)])
def test_ragged_batch_rows_equal_rows_run_alone(pair):
    rs = A().Resampler(*pair, DEV)
    o, n = RF.ratio(*pair)[:2]
    lens = [o + 1, A().RESAMPLE_TILE * o // n + 1, 9001]
    g = torch.Generator().manual_seed(7)
    pad = torch.rand(3, max(lens) + 5, generator=g) * 2 - 1     # whatever lies past a row's length must not be read
    rows = [torch.from_numpy(RF.noise(L, 50 + r)) for r, L in enumerate(lens)]
    for r, L in enumerate(lens):
        pad[r, :L] = rows[r]
    out, olens = rs(pad.to(DEV), lens)
    assert olens == [RF.out_length(L, *pair) for L in lens] and tuple(out.shape) == (3, max(olens))
    out = out.cpu()
    for r, L in enumerate(lens):
        alone, alens = rs(rows[r].to(DEV))
        assert alens == [olens[r]]
        assert torch.equal(out[r, :olens[r]], alone.cpu()[0]), (pair, L)
        assert bool((out[r, olens[r]:] == 0).all()), (pair, L)
    # rows whose pitch leaves them off the 16-byte grid are staged element by element: the same bits
    shifted, _ = rs(pad[:, 1:].to(DEV), [L - 1 for L in lens])
    for r, L in enumerate(lens):
        alone, alens = rs(rows[r][1:].to(DEV))
        assert torch.equal(shifted.cpu()[r, :alens[0]], alone.cpu()[0]), (pair, L)


def test_second_run_is_bit_identical_and_equal_rates_are_the_identity():
    x = torch.from_numpy(RF.noise(22050, 9)).to(DEV)
    rs = A().resampler(22050, 16000, DEV)
    assert rs is A().resampler(22050, 16000, DEV)
    a, _ = rs(x)
    b, _ = rs(x.clone())
    assert torch.equal(a, b)
    c, lens = A().resample(x, 22050, 16000)
    assert torch.equal(a, c) and lens == [16000]
    same, l2 = A().resample(x, 22050, 22050, [22050])
    assert same is x and l2 == [22050]
    assert A().Resampler(16000, 16000, DEV)(x)[0] is x


def test_error_paths_raise_without_a_launch():
    from cosyvoice_lora_finetune_framework_amd.hipops import functional as HF
    from cosyvoice_lora_finetune_framework_amd.hipops.binding import CvftError
    rs = A().Resampler(16000, 22050, DEV)
    x = torch.from_numpy(RF.noise(3001, 2))
    with pytest.raises(CvftError):
        rs(x)
    with pytest.raises(CvftError):
        A().resample(x, 16000, 22050)
    with pytest.raises(ValueError, match="2 lengths for 1 rows"):
        rs(x.to(DEV), [3001, 3001])
    with pytest.raises(ValueError, match="row 0"):
        rs(x.to(DEV), [3002])
    with pytest.raises(NotImplementedError, match="16000"):
        A().extractor(DEV)(x.to(DEV), sample_rate=16000)
    xd = x.to(DEV).reshape(1, -1)
    M = RF.out_length(3001, 16000, 22050)
    for span in (0, 2 * rs.width + 2):
        with pytest.raises(CvftError, match="span"):
            HF.resample(xd, [3001], rs.o, rs.n, rs.width, span, rs.first, rs.taps, M)
    with pytest.raises(CvftError, match="budget"):
        HF.resample(xd, [3001], rs.o, 1000 * rs.n, rs.width, rs.span, rs.first, rs.taps, M)
    torch.cuda.synchronize()
    got, lens = rs(xd)
    assert lens == [M] and torch.equal(got, HF.resample(xd, [3001], rs.o, rs.n, rs.width, rs.span, rs.first, rs.taps, M))


def _write_pcm16(path, x, rate):
    from cosyvoice_lora_finetune_framework_amd.inference_joint import write_wav
    write_wav(str(path), x, rate=rate)


def test_prepare_joint_data_resamples_other_rates(tmp_path):
    from cosyvoice_lora_finetune_framework_amd import prepare_joint_data as P
    from cosyvoice_lora_finetune_framework_amd.dataset import FlowFinetuneDataset
    ext = A().extractor(DEV)
    rates = [16000, 22050, 48000]
    src = tmp_path / "src"
    src.mkdir()
    lines = []
    for i, rate in enumerate(rates):
        _write_pcm16(src / f"u{i}.wav", torch.from_numpy(RF.noise(rate * 3 // 4 + 17 * i, 20 + i)) * 0.5, rate)
        lines.append(dict(utt=f"u{i}", wav=f"u{i}.wav", text=f"t{i}", text_token=[3, 4 + i], speech_token=[5, 6, 7 + i],
                          utt_embedding=[0.001 * (j + i) for j in range(192)]))
    (src / "m.jsonl").write_text("\n".join(json.dumps(e) for e in lines) + "\n")
    out, r16 = tmp_path / "out", tmp_path / "r16"
    P.main(["--manifest", str(src / "m.jsonl"), "--output-dir", str(out), "--resampled-dir", str(r16),
            "--resampled-rate", "16000"])
    ds = FlowFinetuneDataset(str(out), augmentation=False, verbose=False)
    assert len(ds) == 3
    for i, rate in enumerate(rates):
        wav, got_rate = A().load_wav(str(src / f"u{i}.wav"))
        assert got_rate == rate
        xd = wav.to(DEV)
        y, ylens = A().resample(xd, rate, 22050)
        want = ext(y, ylens, channel_last=True).cpu()[0]
        assert torch.equal(ds[i]["speech_feat"], want), rate
        if rate == 22050:                                # today's path: the extractor on the file's own samples
            assert y is xd
            assert torch.equal(want, ext(xd, channel_last=True, sample_rate=rate).cpu()[0])
        with wave.open(str(r16 / f"u{i}.wav")) as f:
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, 16000)
            assert f.getnframes() == A().resampled_length(wav.shape[0], rate, 16000)
    # without the new options nothing else is written, and the 22 050 Hz file's row is the same
    out2 = tmp_path / "out2"
    P.main(["--manifest", str(src / "m.jsonl"), "--output-dir", str(out2)])
    assert sorted(os.listdir(out2)) == ["data.list", "data_000000.parquet"]
    ds2 = FlowFinetuneDataset(str(out2), augmentation=False, verbose=False)
    assert all(torch.equal(ds2[i]["speech_feat"], ds[i]["speech_feat"]) for i in range(3))


def _joint_models():
    from cosyvoice_lora_finetune_framework_amd import utils as U
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    meta = json.load(open(os.path.join(GOLD, "tiny_meta.json")))
    dmeta = json.load(open(os.path.join(GOLD, "llm_decode_meta.json")))
    llm = build_llm_product(dmeta["tiny"], DEV, Numerics())
    llm.sampling = functools.partial(U.ras_sampling, top_k=1, tau_r=1e9)
    return llm, build_flow_product(meta["flow"], DEV, Numerics()), meta, dmeta


def test_synthesize_with_a_prompt_rate():
    from cosyvoice_lora_finetune_framework_amd.inference_joint import synthesize
    llm, flow, _, _ = _joint_models()
    arr = dict(np.load(os.path.join(GOLD, "llm_decode_tiny.npz")))
    text = arr["i_text"][0].tolist()
    wav16 = torch.from_numpy(RF.noise(2000, 31)) * 0.3                    # 0.125 s at 16 kHz -> 2757 samples, 10 frames
    by_hand, lens = A().resample(wav16.to(DEV), 16000, 22050)
    assert lens == [2757]
    p_tok, p_text = [7, 3, 11, 30, 2], [9, 40]
    g = torch.Generator().manual_seed(12)
    emb = torch.randn(1, 192, generator=g)
    z = torch.randn(1, 80, 400, generator=g).to(DEV)
    kw = dict(seed=0, prompt_speech_token=p_tok, prompt_text=p_text, embedding=emb)
    tok_a, mel_a = synthesize(llm, flow, text, prompt_wav=by_hand[0], **kw)
    T = 10 + mel_a.shape[2]
    kw["noise"] = z[:, :, :T].contiguous()
    tok_a, mel_a = synthesize(llm, flow, text, prompt_wav=by_hand[0], **kw)
    tok_b, mel_b = synthesize(llm, flow, text, prompt_wav=wav16, prompt_rate=16000, **kw)
    assert tok_a == tok_b and torch.equal(mel_a, mel_b)
    # prompt_rate None and 22050 are today's path
    tok_c, mel_c = synthesize(llm, flow, text, prompt_wav=by_hand[0].cpu(), prompt_rate=22050, **kw)
    tok_d, mel_d = synthesize(llm, flow, text, prompt_wav=by_hand[0].cpu(), prompt_rate=None, **kw)
    assert tok_c == tok_d == tok_a and torch.equal(mel_c, mel_a) and torch.equal(mel_d, mel_a)


def test_cli_wav_rate_and_prompt_wav_at_another_rate(tmp_path, monkeypatch):
    from hift_fixtures import shaped_weights
    from cosyvoice_lora_finetune_framework_amd import hift as Hm
    from cosyvoice_lora_finetune_framework_amd.inference_joint import main, pcm16, vocode
    from cosyvoice_lora_finetune_framework_amd.lora import get_merged_state_dict
    llm, flow, meta, dmeta = _joint_models()
    arr = dict(np.load(os.path.join(GOLD, "llm_decode_tiny.npz")))
    ref = dict(np.load(os.path.join(GOLD, "llm_decode_joint.npz")))
    voc = Hm.HiFTGenerator()
    w = np.load(os.path.join(GOLD, "hift_weights.npz"))
    voc.load_state_dict(shaped_weights([(k, tuple(v.shape)) for k, v in voc.state_dict().items()],
                                       (w["classifier_weight"], w["classifier_bias"])), strict=True)
    voc = voc.to(DEV).eval()
    torch.save({k: v.cpu() for k, v in get_merged_state_dict(llm).items()}, tmp_path / "llm.pt")
    torch.save({k: v.cpu() for k, v in get_merged_state_dict(flow).items()}, tmp_path / "flow.pt")
    torch.save({k: v.cpu() for k, v in voc.state_dict().items()}, tmp_path / "hift.pt")
    np.save(tmp_path / "z.npy", ref["z"])
    c = dmeta["tiny"]["build"]
    llm_cfg = dict(text_encoder_input_size=c["text_in"], llm_input_size=c["d"], llm_output_size=c["d"],
                   text_token_size=c["text_vocab"], speech_token_size=c["speech_vocab"], attention_heads=c["heads"],
                   linear_units=c["ff"], text_encoder_blocks=c["text_blocks"], llm_blocks=c["llm_blocks"])
    common = ["--llm", str(tmp_path / "llm.pt"), "--flow", str(tmp_path / "flow.pt"),
              "--text-tokens", ",".join(str(int(t)) for t in arr["i_text"][0]), "--top-k", "1", "--tau-r", "1e9",
              "--llm-config", json.dumps(llm_cfg), "--flow-config", json.dumps(meta["flow"]["build"]),
              "--hift", str(tmp_path / "hift.pt"), "--hift-seed", "5"]
    monkeypatch.chdir(tmp_path)
    main(common + ["--noise", str(tmp_path / "z.npy"), "--out", str(tmp_path / "mel.npy"), "--wav", str(tmp_path / "o16.wav"),
                   "--wav-rate", "16000"])
    mel = np.load(tmp_path / "mel.npy")
    with wave.open(str(tmp_path / "o16.wav")) as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, 16000)
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    vocoded = vocode(voc, torch.from_numpy(mel)[None].to(DEV), seed=5)
    want, lens = A().resample(vocoded, 22050, 16000)
    assert pcm.shape[0] == lens[0] == A().resampled_length(mel.shape[1] * 256, 22050, 16000)
    assert np.array_equal(pcm, pcm16(want[0]))
    # a 48 kHz prompt wav goes through the CLI
    _write_pcm16(tmp_path / "p48.wav", torch.from_numpy(RF.noise(6000, 41)) * 0.3, 48000)
    main(common + ["--seed", "0", "--out", str(tmp_path / "melp.npy"), "--wav", str(tmp_path / "p.wav"),
                   "--prompt-wav", str(tmp_path / "p48.wav"), "--prompt-tokens", "7,3,11,30,2", "--prompt-text-tokens", "9,40"])
    with wave.open(str(tmp_path / "p.wav")) as f:
        assert f.getframerate() == 22050 and f.getnframes() == np.load(tmp_path / "melp.npy").shape[1] * 256
