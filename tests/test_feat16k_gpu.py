"""cvft_feat16k on the GPU against the fp64 restatements of tests/feat16k_fixtures.py: parity of the Whisper log-mel and the
Kaldi fbank on the named signals, the exact floor values, ragged batches, determinism, error paths, and the callers --
prepare_joint_data with model hooks and synthesize with a SpeechFrontend.  Measured deviations: DESIGN.md section 21."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import feat16k_fixtures as FX
from helpers import build_flow_product, build_llm_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOUND = 1e-4                                               # the project's fp32 parity bound


def A():
    from cosyvoice_lora_finetune_framework_amd import audio
    return audio


def _dev(name):
    return torch.from_numpy(FX.signal(name).copy()).to(DEV)


@pytest.mark.parametrize("name", [n for n, _ in FX.CASES + FX.WHISPER_ONLY])
def test_whisper_parity_with_the_fp64_restatement(name):
    """max |gpu - fp64| <= 1e-4 on every named signal."""
    want, d_ref = FX.reference("whisper", name)
    got = A().whisper_log_mel(_dev(name))
    assert tuple(got.shape) == (1,) + want.shape and got.dtype == torch.float32
    err = float(np.abs(got[0].cpu().numpy().astype(np.float64) - want).max())
    print(f"whisper {name}: max |gpu - fp64| = {err:.3e} (fp32 restatement {d_ref:.3e}, bound {BOUND:.0e})")
    assert err <= BOUND, (name, err)


@pytest.mark.parametrize("cmn", [True, False])
@pytest.mark.parametrize("name", [n for n, _ in FX.CASES])
def test_fbank_parity_with_the_fp64_restatement(name, cmn):
    """max |gpu - fp64| <= max(1e-4, 4 d_ref), d_ref the fp32 restatement's own deviation on the case (<= 1e-4 on each): two
    fp32 evaluations that differ only in the order of a 400-term sum."""
    want, d_ref = FX.reference("fbank", name, cmn)
    assert d_ref <= 1e-4
    got = A().kaldi_fbank(_dev(name), cmn=cmn)
    assert tuple(got.shape) == (1,) + want.shape and got.dtype == torch.float32
    err = float(np.abs(got[0].cpu().numpy().astype(np.float64) - want).max())
    bound = max(BOUND, 4.0 * d_ref)
    print(f"fbank cmn={cmn} {name}: max |gpu - fp64| = {err:.3e} (fp32 restatement {d_ref:.3e}, bound {bound:.3e})")
    assert err <= bound, (name, cmn, err, bound)


def test_exact_floor_values():
    # digital silence: log10 of the floor is -10, the row maximum too, so (-10 + 4) / 4 everywhere
    z = A().whisper_log_mel(torch.zeros(2, 720, device=DEV), [720, 500])
    assert tuple(z.shape) == (2, 128, 4)
    assert bool((z[0] == -1.5).all()) and bool((z[1, :, :3] == -1.5).all()) and bool((z[1, :, 3:] == 0).all())
    # frames 34 .. 43 of the gapped signal lie inside the zeroed samples 5333 .. 7332
    raw = A().kaldi_fbank(_dev("16000z"), cmn=False)[0].cpu().numpy()
    floor = np.log(np.float32(1.1920929e-07))
    assert floor.dtype == np.float32 and floor == FX.K_FLOOR
    assert (raw[34:44] == floor).all() and (raw[:33] > floor).all() and (raw[45:] > floor).all()
    assert bool((A().kaldi_fbank(torch.zeros(1, 900, device=DEV), cmn=False) == float(floor)).all())
    assert bool((A().kaldi_fbank(torch.zeros(1, 900, device=DEV)) == 0).all())         # minus its own mean


@pytest.mark.parametrize("feature", ["whisper", "fbank", "fbank_raw"])
def test_ragged_batch_rows_equal_rows_run_alone(feature):
    names = ["16000z", "559", "10400"]
    lens = [FX.signal(n).shape[0] for n in names]
    g = torch.Generator().manual_seed(3)
    pad = torch.rand(3, max(lens) + 7, generator=g) * 2 - 1            # whatever lies past a row's length must not be read
    for r, n in enumerate(names):
        pad[r, :lens[r]] = torch.from_numpy(FX.signal(n).copy())
    if feature == "whisper":
        run, count = A().whisper_log_mel, FX.whisper_frames
        frames = lambda o, r, T: o[r, :, :T]                          # noqa: E731
        rest = lambda o, r, T: o[r, :, T:]                            # noqa: E731
    else:
        run, count = functools.partial(A().kaldi_fbank, cmn=feature == "fbank"), FX.fbank_frames
        frames = lambda o, r, T: o[r, :T]                             # noqa: E731
        rest = lambda o, r, T: o[r, T:]                               # noqa: E731
    x = pad.to(DEV)
    out = run(x, lens)
    again = run(x.clone(), lens)
    assert torch.equal(out, again)                                     # a second call is bit-identical
    assert out.shape[2 if feature == "whisper" else 1] == count(max(lens))
    for r, n in enumerate(names):
        alone = run(_dev(n))
        T = count(lens[r])
        assert torch.equal(frames(out, r, T), frames(alone, 0, T)), (feature, n)
        assert bool((rest(out, r, T) == 0).all()), (feature, n)
    assert A().whisper_extractor(DEV) is A().whisper_extractor(DEV) and A().fbank_extractor(DEV) is A().fbank_extractor(DEV)


def test_error_paths_raise_without_a_launch():
    from cosyvoice_lora_finetune_framework_amd.hipops import functional as HF
    from cosyvoice_lora_finetune_framework_amd.hipops.binding import CvftError
    x = _dev("720").reshape(1, -1)
    with pytest.raises(CvftError):
        A().whisper_log_mel(x.cpu())
    with pytest.raises(CvftError):
        A().kaldi_fbank(x.cpu())
    with pytest.raises(ValueError, match="row 0: 399"):
        A().kaldi_fbank(x, [399])
    with pytest.raises(ValueError, match="row 0: 200"):
        A().whisper_log_mel(x, [200])
    w, f = A().whisper_extractor(DEV), A().fbank_extractor(DEV)
    with pytest.raises(ValueError, match="fp32"):
        HF.feat16k(0, x.double(), [720], w.dft_tab, w.basis_tab, w.nchunks, 4)
    with pytest.raises(CvftError):
        HF.feat16k(0, x, [720], w.dft_tab.cpu(), w.basis_tab, w.nchunks, 4)
    with pytest.raises(ValueError, match="tables"):
        HF.feat16k(1, x, [720], w.dft_tab, w.basis_tab, f.nchunks, 3)
    with pytest.raises(ValueError, match="kind"):
        HF.feat16k(2, x, [720], w.dft_tab, w.basis_tab, w.nchunks, 4)
    with pytest.raises(ValueError, match="lengths"):
        HF.feat16k(1, x, [721], f.dft_tab, f.basis_tab, f.nchunks, 3)
    torch.cuda.synchronize()
    assert torch.equal(HF.feat16k(1, x, [720], f.dft_tab, f.basis_tab, f.nchunks, 3), A().kaldi_fbank(x))


# ---- callers ------------------------------------------------------------------------------
class _StandIns:
    """The two external models as plain callables: they keep what they were fed and answer from it alone."""

    def __init__(self):
        self.tok_feats, self.emb_feats = {}, {}

    def tokenizer(self, feat, length):
        assert isinstance(feat, np.ndarray) and feat.dtype == np.float32 and feat.shape == (1, 128, int(length))
        self.tok_feats[int(length)] = feat.copy()
        return [int(length) % 97 + 1, 7, int(abs(float(feat.sum()))) % 50]

    def encoder(self, feat):
        assert isinstance(feat, np.ndarray) and feat.dtype == np.float32 and feat.shape[0] == 1 and feat.shape[2] == 80
        self.emb_feats[feat.shape[1]] = feat.copy()
        return (np.arange(192, dtype=np.float32) * 1e-3 + np.float32(feat[0, 0, :5].sum())).tolist()


def test_prepare_joint_data_fills_tokens_and_embeddings(tmp_path):
    import pyarrow.parquet as pq
    from cosyvoice_lora_finetune_framework_amd import prepare_joint_data as P
    from cosyvoice_lora_finetune_framework_amd.inference_joint import write_wav
    src = tmp_path / "src"
    src.mkdir()
    files = [(16000, 8800), (48000, 27500), (48000, 29000)]             # 0.55 s .. 0.6 s: above the duration filter
    lines = []
    for i, (rate, n) in enumerate(files):
        write_wav(str(src / f"u{i}.wav"), torch.from_numpy(FX.base_signal(n, 70 + i)), rate)
        lines.append(dict(utt=f"u{i}", wav=f"u{i}.wav", text=f"t{i}", text_token=[3, 4 + i]))
    (src / "m.jsonl").write_text("\n".join(json.dumps(e) for e in lines) + "\n")
    with pytest.raises(ValueError, match="missing speech_token, utt_embedding"):
        P.prepare(str(src / "m.jsonl"), str(tmp_path / "none"), verbose=False)
    m = _StandIns()
    shards = P.prepare(str(src / "m.jsonl"), str(tmp_path / "out"), verbose=False, speech_tokenizer=m.tokenizer,
                       speaker_encoder=m.encoder)
    rows = {r["utt"]: r for r in pq.read_table(shards[0]).to_pylist()}
    assert len(m.tok_feats) == 3 and len(m.emb_feats) == 3
    direct = {}
    for i, (rate, n) in enumerate(files):
        wav, got_rate = A().load_wav(str(src / f"u{i}.wav"))
        assert got_rate == rate and wav.shape[0] == n
        w16, lens = A().resample(wav.to(DEV), rate, 16000)
        w16 = w16.reshape(1, -1)
        T, M = A().whisper_frames(w16.shape[1]), A().fbank_frames(w16.shape[1])
        mel, fb = A().whisper_log_mel(w16).cpu().numpy(), A().kaldi_fbank(w16).cpu().numpy()
        # the callables received exactly what a direct call on the resampled audio gives
        assert np.array_equal(m.tok_feats[T], mel) and np.array_equal(m.emb_feats[M], fb)
        direct[i] = (mel, fb)
        row = rows[f"u{i}"]
        assert row["speech_token"] == m.tokenizer(mel, T)
        assert np.array_equal(np.asarray(row["utt_embedding"], dtype=np.float32), np.asarray(m.encoder(fb), dtype=np.float32))
        assert row["spk_embedding"] == row["utt_embedding"]
    # a manifest that carries the keys keeps them, and the models are not asked for those rows
    lines[1].update(speech_token=[9, 8, 7], utt_embedding=[0.25] * 192)
    lines[2].update(speech_token=[5])
    (src / "m2.jsonl").write_text("\n".join(json.dumps(e) for e in lines) + "\n")
    m2 = _StandIns()
    shards = P.prepare(str(src / "m2.jsonl"), str(tmp_path / "out2"), verbose=False, speech_tokenizer=m2.tokenizer,
                       speaker_encoder=m2.encoder)
    rows2 = {r["utt"]: r for r in pq.read_table(shards[0]).to_pylist()}
    assert rows2["u1"]["speech_token"] == [9, 8, 7] and rows2["u1"]["utt_embedding"] == [0.25] * 192
    assert rows2["u2"]["speech_token"] == [5] and rows2["u2"]["utt_embedding"] == rows["u2"]["utt_embedding"]
    assert rows2["u0"]["speech_token"] == rows["u0"]["speech_token"]
    assert len(m2.tok_feats) == 1 and len(m2.emb_feats) == 2
    assert all(rows2[u]["speech_feat"] == rows[u]["speech_feat"] for u in rows)
    # only a tokenizer: utt_embedding stays required
    with pytest.raises(ValueError, match="missing utt_embedding"):
        P.prepare(str(src / "m.jsonl"), str(tmp_path / "out3"), verbose=False, speech_tokenizer=m.tokenizer)


def _joint_models():
    from cosyvoice_lora_finetune_framework_amd import utils as U
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    meta = json.load(open(os.path.join(GOLD, "tiny_meta.json")))
    dmeta = json.load(open(os.path.join(GOLD, "llm_decode_meta.json")))
    llm = build_llm_product(dmeta["tiny"], DEV, Numerics())
    llm.sampling = functools.partial(U.ras_sampling, top_k=1, tau_r=1e9)
    return llm, build_flow_product(meta["flow"], DEV, Numerics())


def test_synthesize_with_a_speech_frontend():
    from cosyvoice_lora_finetune_framework_amd.frontend16k import SpeechFrontend
    from cosyvoice_lora_finetune_framework_amd.inference_joint import synthesize
    llm, flow = _joint_models()
    text = dict(np.load(os.path.join(GOLD, "llm_decode_tiny.npz")))["i_text"][0].tolist()
    wav16 = torch.from_numpy(FX.base_signal(2000, 31)) * 0.5              # 0.125 s at 16 kHz: 12 / 11 frames
    p_tok, p_text = [7, 3, 11, 30, 2], [9, 40]
    g = torch.Generator().manual_seed(12)
    emb = torch.randn(1, 192, generator=g)
    z = torch.randn(1, 80, 400, generator=g).to(DEV)
    seen = {}

    def tokenizer(feat, length):
        seen["tok"] = (feat.copy(), int(length))
        return list(p_tok)

    def encoder(feat):
        seen["emb"] = feat.copy()
        return emb.reshape(-1).tolist()

    fe = SpeechFrontend(DEV, tokenizer, encoder)
    assert fe.tokens(wav16) == [p_tok] and torch.equal(fe.embeddings(wav16), emb)
    assert seen["tok"][1] == 12 and np.array_equal(seen["tok"][0], A().whisper_log_mel(wav16.to(DEV)).cpu().numpy())
    assert seen["emb"].shape == (1, 11, 80) and np.array_equal(seen["emb"], A().kaldi_fbank(wav16.to(DEV)).cpu().numpy())
    kw = dict(seed=0, prompt_text=p_text, prompt_wav=wav16, prompt_rate=16000)
    _, mel0 = synthesize(llm, flow, text, prompt_speech_token=p_tok, embedding=emb, **kw)
    kw["noise"] = z[:, :, :10 + mel0.shape[2]].contiguous()
    tok_a, mel_a = synthesize(llm, flow, text, prompt_speech_token=p_tok, embedding=emb, **kw)
    tok_b, mel_b = synthesize(llm, flow, text, frontend=fe, **kw)
    assert tok_a == tok_b and torch.equal(mel_a, mel_b)
    # an explicit value still wins over the frontend's
    other = SpeechFrontend(DEV, lambda feat, length: [1, 2], lambda feat: [0.5] * 192)
    tok_c, mel_c = synthesize(llm, flow, text, frontend=other, prompt_speech_token=p_tok, embedding=emb, **kw)
    assert tok_c == tok_a and torch.equal(mel_c, mel_a)
