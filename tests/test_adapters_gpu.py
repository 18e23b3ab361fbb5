"""Per-request LoRA adapters at inference on the GPU: the two adapter kernels of csrc/decode.hip against fp64
restatements of their fp32 / bf16 operands, and TransformerLM.inference / inference_batch, inference_joint.synthesize, the
CLI and StreamingSynthesizer.tts over an adapters.AdapterBank against the golden decode fixtures (the reference's own
unmerged run) and against models that took the same adapter through load_lora_weights."""
import copy
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import build_flow_product, build_llm_product, rel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S = 3                                   # slots in the op tests
SLOTS = [1, -1, 0, 2, S, 2, 7, 0, 1, -5, 2, 0, 1, 1, -1, 2]          # mixed: valid, -1, out of range


def _ops():
    from cosyvoice_lora_finetune_framework_amd import decode as D
    return D


def _ln64(x, lg, lb, eps=1e-5):
    x64 = x.double()
    xn = (x64 - x64.mean(1, keepdim=True)) / torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + eps)
    return xn * lg.double() + lb.double()


def _slots(M, shift=0):
    return [SLOTS[(i + shift) % len(SLOTS)] for i in range(M)]


# ------------------------------------------------------------------------------------------------ down-projection
@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", [128, 1024, 4096])
def test_lora_down_vs_fp64(K, wdt):
    D = _ops()
    g = torch.Generator(device="cpu").manual_seed(K + 3)
    lg, lb = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    for R in (8, 64):
        for G in (1, 3):
            A = (torch.randn(S, G, R, K, generator=g) / math.sqrt(K)).to(wdt)
            Ad = A.to(DEV)
            for M in (1, 3, 16):
                X = torch.randn(M, K, generator=g) * 2 + 0.5
                for shift in ((0, 1) if M == 1 else (0,)):                 # M = 1: a valid slot, then slot -1
                    sl = _slots(M, shift)
                    sd = torch.tensor(sl, dtype=torch.int32, device=DEV)
                    for ln in (None, (lg.to(DEV), lb.to(DEV), 1e-5)):
                        z = D.decode_lora_down(X.to(DEV), Ad, sd, ln=ln)
                        torch.cuda.synchronize()
                        x64 = X.double() if ln is None else _ln64(X, lg, lb)
                        for m, s in enumerate(sl):
                            if 0 <= s < S:
                                ref = torch.cat([A[s, gg].double() @ x64[m] for gg in range(G)])
                                assert rel(z[m], ref) < 1e-5, (R, G, M, m, ln is not None, rel(z[m], ref))
                            else:
                                assert torch.equal(z[m].cpu(), torch.zeros(G * R)), (R, G, M, m)


# ------------------------------------------------------------------------------------------------ linear + up-projection
LIN = [(128, 51, 1), (1024, 3072, 3), (1024, 4097, 1), (4096, 1024, 1)]


def _lin_operands(K, N, G, R, wdt, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(wdt)
    Bst = (torch.randn(S, N, R, generator=g) / math.sqrt(R)).to(wdt)
    scale = torch.tensor([2.0, 0.375, 1.3])
    b = torch.randn(N, generator=g) * 0.1
    lg, lb = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    return g, W, Bst, scale, b, lg, lb


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,N,G", LIN)
def test_linear_lora_vs_fp64(K, N, G, wdt):
    D = _ops()
    for R in (8, 64):
        g, W, Bst, scale, b, lg, lb = _lin_operands(K, N, G, R, wdt, K * 7 + N + R)
        Wd, Bd, sc = W.to(DEV), Bst.to(DEV), scale.to(DEV)
        Ng = N // G
        for M in (1, 3, 16):
            X = torch.randn(M, K, generator=g) * 2 + 0.5
            Z = torch.randn(M, G * R, generator=g)
            Rs = torch.randn(M, N, generator=g)
            sl = _slots(M)
            sd = torch.tensor(sl, dtype=torch.int32, device=DEV)
            up = torch.zeros(M, N, dtype=torch.float64)
            for m, s in enumerate(sl):
                if 0 <= s < S:
                    for gg in range(G):
                        up[m, gg * Ng:(gg + 1) * Ng] = scale[s].double() * (
                            Bst[s, gg * Ng:(gg + 1) * Ng].double() @ Z[m, gg * R:(gg + 1) * R].double())
            x64, w64 = X.double(), W.double()
            ln = (lg.to(DEV), lb.to(DEV), 1e-5)
            plain = D.decode_linear_lora(X.to(DEV), Wd, Bd, sc, sd, Z.to(DEV), G)
            assert rel(plain, x64 @ w64.T + up) < 1e-5, (R, M, "plain")
            y = D.decode_linear_lora(X.to(DEV), Wd, Bd, sc, sd, Z.to(DEV), G, bias=b.to(DEV), ln=ln, act=1)
            assert rel(y, torch.relu(_ln64(X, lg, lb) @ w64.T + b.double() + up)) < 1e-5, (R, M, "bias_relu_ln")
            h = Rs.to(DEV).clone()                                       # the residual aliases Y
            D.decode_linear_lora(X.to(DEV), Wd, Bd, sc, sd, Z.to(DEV), G, bias=b.to(DEV), residual=h, out=h)
            torch.cuda.synchronize()
            assert rel(h, x64 @ w64.T + b.double() + up + Rs.double()) < 1e-5, (R, M, "bias_residual")


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,N,G", [(128, 51, 1), (1024, 3072, 3)])
def test_rows_without_adapter_are_decode_linear_and_rows_are_independent(K, N, G, wdt):
    D = _ops()
    R, M = 16, 16
    g, W, Bst, scale, b, lg, lb = _lin_operands(K, N, G, R, wdt, 91 + N)
    A = (torch.randn(S, G, R, K, generator=g) / math.sqrt(K)).to(wdt).to(DEV)
    Wd, Bd, sc, bd = W.to(DEV), Bst.to(DEV), scale.to(DEV), b.to(DEV)
    ln = (lg.to(DEV), lb.to(DEV), 1e-5)
    X = (torch.randn(M, K, generator=g) * 2 + 0.5).to(DEV)
    Rs = torch.randn(M, N, generator=g).to(DEV)
    sl = _slots(M)
    sd = torch.tensor(sl, dtype=torch.int32, device=DEV)
    z = D.decode_lora_down(X, A, sd, ln=ln)
    y = D.decode_linear_lora(X, Wd, Bd, sc, sd, z, G, bias=bd, ln=ln, act=1, residual=Rs)
    base = D.decode_linear(X, Wd, bias=bd, ln=ln, act=1, residual=Rs)
    torch.cuda.synchronize()
    differs = 0
    for m, s in enumerate(sl):
        one = torch.tensor([s], dtype=torch.int32, device=DEV)
        z1 = D.decode_lora_down(X[m:m + 1], A, one, ln=ln)
        y1 = D.decode_linear_lora(X[m:m + 1], Wd, Bd, sc, one, z1, G, bias=bd, ln=ln, act=1, residual=Rs[m:m + 1])
        assert torch.equal(z1[0], z[m]) and torch.equal(y1[0], y[m]), m          # alone (M = 1) == inside the mixed batch
        if 0 <= s < S:
            differs += int(not torch.equal(y[m], base[m]))
        else:
            assert torch.equal(y[m], base[m]), m                                   # no adapter: cvft_decode_linear, bit for bit
    assert differs == sum(0 <= s < S for s in sl)


# ------------------------------------------------------------------------------------------------ models
def _meta():
    return json.load(open(os.path.join(GOLD, "llm_decode_meta.json")))["tiny"]


def _arr():
    return dict(np.load(os.path.join(GOLD, "llm_decode_tiny.npz")))


def _greedy():
    from cosyvoice_lora_finetune_framework_amd import utils as U
    return functools.partial(U.ras_sampling, top_k=1, tau_r=1e9)


def _case(arr, k):
    t = lambda n: torch.from_numpy(arr[f"{k}_{n}"])           # noqa: E731
    text, ptext, ptok, emb = t("text"), t("ptext"), t("ptok"), t("emb")
    return (text.to(DEV), torch.tensor([text.shape[1]]), ptext.to(DEV), torch.tensor([ptext.shape[1]]), ptok.to(DEV),
            torch.tensor([ptok.shape[1]]), emb.to(DEV))


B_R, B_ALPHA = 8, 6.0                   # adapter "b": rank 8, scale 0.75 (the models' own LoRA: r 4, alpha 8)


def _random_adapter(model, r, seed):
    """a seeded random adapter of rank r for every LoRA layer of `model` (state-dict names, CPU)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for n, p in model.named_parameters():
        if "lora_A" in n:
            sd[n] = torch.randn(r, *p.shape[1:], generator=g) / math.sqrt(p.shape[1])
        elif "lora_B" in n:
            sd[n] = torch.randn(p.shape[0], r, *p.shape[2:], generator=g) * 0.05
    return sd


def _zero_lora(model):
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "lora_" in n:
                p.zero_()


@functools.lru_cache(maxsize=None)
def _adapters():
    """("gold": the golden model's own LoRA tensors, "b": seeded random, rank 8) as CPU state dicts."""
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    m = build_llm_product(_meta(), torch.device("cpu"), Numerics())
    gold = {n: p.detach().clone() for n, p in m.named_parameters() if "lora_" in n}
    return gold, _random_adapter(m, B_R, 4242)


def _bank_model(capacity=4, dtype=torch.float32, sampling="greedy"):
    """the tiny model with every LoRA parameter zeroed, and a bank of rank 8 over it holding "gold" and "b"."""
    from cosyvoice_lora_finetune_framework_amd.adapters import AdapterBank
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    m = build_llm_product(_meta(), DEV, Numerics(dtype=dtype))
    m.sampling = _greedy() if sampling == "greedy" else None
    _zero_lora(m)
    bank = AdapterBank(llm=m, capacity=capacity, rank=8)
    gold, b = _adapters()
    bank.load("gold", gold)
    bank.load("b", b, alpha=B_ALPHA)
    return m, bank


def _merged_model(adapter, tmp_path, sampling="greedy"):
    """a model that took the adapter through load_lora_weights (merged decode path); adapter None: LoRA zeroed."""
    from cosyvoice_lora_finetune_framework_amd.lora import load_lora_weights
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    meta = copy.deepcopy(_meta())
    if adapter is not None:
        meta["lora"].update(r=B_R, alpha=B_ALPHA)
    m = build_llm_product(meta, DEV, Numerics())
    m.sampling = _greedy() if sampling == "greedy" else None
    if adapter is None:
        _zero_lora(m)
    else:
        torch.save(adapter, tmp_path / "b_llm.pt")
        load_lora_weights(m, str(tmp_path / "b_llm.pt"))
    return m


def _session(m):
    return list(m._cvft_sessions.values())[-1][1]            # the most recently used one


@pytest.mark.parametrize("case", ["i", "ii"])
def test_adapter_path_reproduces_the_golden_decode(case):
    arr = _arr()
    m, _ = _bank_model()
    ref, lp = arr[f"{case}_tokens"].tolist(), arr[f"{case}_lp"]
    toks, dev_lp = [], []
    for t in m.inference(*_case(arr, case), adapter="gold"):
        toks.append(t)
        dev_lp.append(_session(m).logp[0].cpu())
    assert toks == ref
    want = torch.from_numpy(lp[:len(dev_lp)]).double()
    d = (torch.stack(dev_lp).double() - want).abs()
    assert float((d / want.abs().clamp_min(1.0)).max()) <= 1e-4


FORCED = 32


def _forced_logp(m, args, tokens, **kw):
    """teacher-force `tokens` through the host-callable sampler path; -> the device's logp of every step [steps, V]."""
    lps = []

    def sampler(scores, decoded, sampling):
        lps.append(_session(m).logp[0].double().cpu())
        return torch.tensor([tokens[len(decoded)]])
    keep, m.sampling = m.sampling, sampler
    try:
        n_text = int(args[1])
        out = list(m.inference(*args, max_token_text_ratio=(len(tokens) + 0.5) / n_text, min_token_text_ratio=0, **kw))
    finally:
        m.sampling = keep
    assert out == list(tokens)
    return torch.stack(lps)


def _lp_err(a, b):
    return float(((a - b).abs() / b.abs().clamp_min(1.0)).max())


def test_second_adapter_and_base_match_the_merged_path(tmp_path):
    from cosyvoice_lora_finetune_framework_amd.adapters import BASE
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    arr = _arr()
    args = _case(arr, "ii")
    V = _meta()["build"]["speech_vocab"]
    tokens = torch.randint(0, V, (FORCED,), generator=torch.Generator().manual_seed(17)).tolist()
    m, _ = _bank_model()
    _, b = _adapters()
    lp_b = _forced_logp(m, args, tokens, adapter="b")
    lp_base = _forced_logp(m, args, tokens, adapter=BASE)
    want_b = _forced_logp(_merged_model(b, tmp_path), args, tokens)
    want_base = _forced_logp(_merged_model(None, tmp_path), args, tokens)
    print("adapter b vs merged", _lp_err(lp_b, want_b), "BASE vs merged", _lp_err(lp_base, want_base),
          "b vs base", _lp_err(want_b, want_base))
    assert _lp_err(lp_b, want_b) <= 1e-4
    assert _lp_err(lp_base, want_base) <= 1e-4
    assert _lp_err(want_b, want_base) > 1e-2                      # the adapter matters: the two checks are not one
    # bf16 weights: logp[token fed] per step against the fp32 adapter path (the bf16 bar of the full-size decode test)
    m.numerics = Numerics(dtype=torch.bfloat16)
    lp_bf = _forced_logp(m, args, tokens, adapter="b")
    idx = torch.tensor(tokens)
    err = (lp_bf[torch.arange(FORCED), idx] - lp_b[torch.arange(FORCED), idx]).abs()
    print("bf16 adapter path |dlogp| max", float(err.max()), "mean", float(err.mean()))
    assert float(err.max()) <= 0.05


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_mixed_batch_equals_single_runs(sampled):
    from cosyvoice_lora_finetune_framework_amd.adapters import BASE
    m, _ = _bank_model(sampling="ras" if sampled else "greedy")
    g = torch.Generator(device="cpu").manual_seed(77)
    texts = [torch.randint(0, 100, (n,), generator=g) for n in (4, 2, 3, 1)]
    embs = [torch.zeros(1, 192), torch.randn(1, 192, generator=g), torch.zeros(0, 192), torch.randn(1, 192, generator=g)]
    seeds = [101, 202, 303, 404]
    names = ["gold", "b", BASE, "gold"]
    batch = m.inference_batch([t.to(DEV) for t in texts], embeddings=[e.to(DEV) for e in embs], seeds=seeds,
                              min_token_text_ratio=0.5, adapters=names)
    z = torch.zeros(1, 0, dtype=torch.long, device=DEV)
    singles = []
    for b in range(4):
        singles.append(list(m.inference(texts[b][None].to(DEV), torch.tensor([texts[b].numel()]), z, torch.tensor([0]), z,
                                        torch.tensor([0]), embs[b].to(DEV), min_token_text_ratio=0.5, seed=seeds[b],
                                        adapter=names[b])))
        assert batch[b] == singles[b], b
    assert len({tuple(s) for s in singles}) > 1


def test_adapters_come_and_go_under_one_pack_session_and_graph():
    from cosyvoice_lora_finetune_framework_amd.adapters import AdapterBank
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    arr = _arr()
    args = _case(arr, "i")
    m = build_llm_product(_meta(), DEV, Numerics())
    m.sampling = _greedy()
    _zero_lora(m)
    gold, b = _adapters()
    bank = AdapterBank(llm=m, capacity=2, rank=8)

    def run(name):
        toks = list(m.inference(*args, adapter=name))
        s = _session(m)
        return toks, s.logits.clone(), (m._cvft_decode_weights[(torch.float32, "unfolded")][1], s, s.graph)

    bank.load("gold", gold)
    t1, l1, objs = run("gold")
    assert t1 == arr["i_tokens"].tolist() and objs[2] is not None
    bank.load("b", b, alpha=B_ALPHA)
    bank.load("c", _random_adapter(m, 4, 5))                       # a full bank: "gold", the least recently used, goes
    assert bank.names() == ["b", "c"]
    tb, _, objs_b = run("b")
    assert bank.load("gold", gold) == bank.slot("gold") and bank.names() == ["b", "gold"]
    t2, l2, objs2 = run("gold")
    assert all(x is y for x, y in zip(objs, objs_b)) and all(x is y for x, y in zip(objs, objs2))
    assert len(m._cvft_sessions) == 1
    assert t2 == t1 and torch.equal(l1, l2) and tb != t1


def test_adapter_graph_decode_bit_identical_to_eager():
    arr = _arr()
    m, _ = _bank_model(sampling="ras")
    args = _case(arr, "i")
    runs = []
    for use_graph in (True, False):
        toks = []
        for t in m.inference(*args, seed=1234, use_graph=use_graph, min_token_text_ratio=20, adapter="gold"):
            toks.append(t)
            if len(toks) == 64:
                runs.append((toks, _session(m).logits.cpu().clone()))
                break
    assert len(runs) == 2 and len(runs[0][0]) == 64
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------ joint
FLOW_ALPHA = 12.0


@functools.lru_cache(maxsize=None)
def _joint():
    """(llm + flow over one bank holding "b", the pair of models that took "b" through load_lora_weights, files)."""
    import tempfile
    from cosyvoice_lora_finetune_framework_amd.adapters import AdapterBank
    from cosyvoice_lora_finetune_framework_amd.lora import load_lora_weights
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    tmp = tempfile.mkdtemp()
    fmeta = json.load(open(os.path.join(GOLD, "tiny_meta.json")))["flow"]
    llm = build_llm_product(_meta(), DEV, Numerics())
    flow = build_flow_product(fmeta, DEV, Numerics())
    _, b_llm = _adapters()
    b_flow = _random_adapter(flow, B_R, 777)
    torch.save(b_llm, os.path.join(tmp, "b_llm.pt"))
    torch.save(b_flow, os.path.join(tmp, "b_flow.pt"))
    base = lambda mod: {k.replace(".original_layer", ""): v.detach().cpu().clone()          # noqa: E731
                        for k, v in mod.state_dict().items() if "lora_" not in k}
    torch.save(base(llm), os.path.join(tmp, "llm_base.pt"))
    torch.save(base(flow), os.path.join(tmp, "flow_base.pt"))
    _zero_lora(llm)
    _zero_lora(flow)
    llm.sampling = None
    bank = AdapterBank(llm=llm, flow=flow, capacity=2, rank=8)
    bank.load("b", os.path.join(tmp, "b_llm.pt"), alpha=B_ALPHA)
    bank.load("b", os.path.join(tmp, "b_flow.pt"), alpha=FLOW_ALPHA)
    m8, f8 = copy.deepcopy(_meta()), copy.deepcopy(fmeta)
    m8["lora"].update(r=B_R, alpha=B_ALPHA)
    f8["lora"].update(r=B_R, alpha=FLOW_ALPHA)
    llm8 = build_llm_product(m8, DEV, Numerics())
    flow8 = build_flow_product(f8, DEV, Numerics())
    load_lora_weights(llm8, os.path.join(tmp, "b_llm.pt"))
    load_lora_weights(flow8, os.path.join(tmp, "b_flow.pt"))
    llm8.sampling = None
    return llm, flow, llm8, flow8, tmp


def _pinned(seed=31):
    """the pair's tokens and mel of case i's text under a pinned seed and noise."""
    from cosyvoice_lora_finetune_framework_amd.inference_joint import synthesize
    llm, flow, llm8, flow8, _ = _joint()
    text = _arr()["i_text"][0].tolist()
    _, probe = synthesize(llm8, flow8, text, seed=seed)
    z = torch.randn(probe.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    tokens, mel = synthesize(llm8, flow8, text, seed=seed, noise=z)
    return text, z, tokens, mel


def test_joint_synthesize_with_an_adapter_equals_the_loaded_pair():
    from cosyvoice_lora_finetune_framework_amd.adapters import BASE
    from cosyvoice_lora_finetune_framework_amd.inference_joint import synthesize
    llm, flow, _, _, _ = _joint()
    text, z, tokens, mel = _pinned()
    got_t, got_mel = synthesize(llm, flow, text, seed=31, noise=z, adapter="b")
    assert got_t == tokens
    assert torch.equal(got_mel, mel)
    base_t, _ = synthesize(llm, flow, text, seed=31, adapter=BASE)
    assert base_t != tokens


def test_joint_cli_serves_a_voice_from_base_weights(tmp_path):
    from cosyvoice_lora_finetune_framework_amd.inference_joint import main
    _, _, _, _, tmp = _joint()
    text, z, tokens, mel = _pinned()
    meta = json.load(open(os.path.join(GOLD, "tiny_meta.json")))
    c = _meta()["build"]
    llm_cfg = dict(text_encoder_input_size=c["text_in"], llm_input_size=c["d"], llm_output_size=c["d"],
                   text_token_size=c["text_vocab"], speech_token_size=c["speech_vocab"], attention_heads=c["heads"],
                   linear_units=c["ff"], text_encoder_blocks=c["text_blocks"], llm_blocks=c["llm_blocks"])
    lora = lambda L, alpha: json.dumps(dict(lora_r=B_R, lora_alpha=alpha, target_modules=L["targets"]))      # noqa: E731
    np.save(tmp_path / "z.npy", z.cpu().numpy())
    out = tmp_path / "mel.npy"
    main(["--llm", os.path.join(tmp, "llm_base.pt"), "--flow", os.path.join(tmp, "flow_base.pt"),
          "--lora", "b=" + os.path.join(tmp, "b_llm.pt"), "--lora", "b=" + os.path.join(tmp, "b_flow.pt"), "--voice", "b",
          "--llm-lora-config", lora(_meta()["lora"], B_ALPHA), "--flow-lora-config", lora(meta["flow"]["lora"], FLOW_ALPHA),
          "--text-tokens", ",".join(str(int(t)) for t in text), "--out", str(out), "--seed", "31",
          "--llm-config", json.dumps(llm_cfg), "--flow-config", json.dumps(meta["flow"]["build"]),
          "--noise", str(tmp_path / "z.npy")])
    assert torch.equal(torch.from_numpy(np.load(out)), mel[0].cpu())


def test_streaming_with_an_adapter_equals_streaming_from_the_loaded_pair():
    from hift_fixtures import shaped_weights
    from cosyvoice_lora_finetune_framework_amd.hift import HiFTGenerator
    from cosyvoice_lora_finetune_framework_amd.streaming import StreamingSynthesizer
    hift = HiFTGenerator()
    w = np.load(os.path.join(GOLD, "hift_weights.npz"))
    spec = [(k, tuple(v.shape)) for k, v in hift.state_dict().items()]
    hift.load_state_dict(shaped_weights(spec, (w["classifier_weight"], w["classifier_bias"])), strict=True)
    hift = hift.to(DEV).eval()
    llm, flow, llm8, flow8, _ = _joint()
    text = _arr()["i_text"][0].tolist()
    ratio = 90.5 / len(text)
    kw = dict(min_token_text_ratio=ratio, max_token_text_ratio=ratio)

    def run(a, b, **extra):
        syn = StreamingSynthesizer(a, b, hift, token_hop_len=20, token_max_hop_len=20)
        torch.manual_seed(1234)
        return [it["tts_speech"] for it in syn.tts(text, stream=True, seed=7, hift_seed=11, llm_kw=kw, **extra)]
    want = run(llm8, flow8)
    got = run(llm, flow, adapter="b")
    assert len(want) == len(got) == 4
    assert all(torch.equal(x, y) for x, y in zip(got, want))
