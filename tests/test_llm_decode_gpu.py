"""Autoregressive speech-token generation on the GPU: the decode kernels against fp64 restatements, and
TransformerLM.forward_chunk / inference / inference_batch against the reference's own outputs
(tests/golden/llm_decode_*.npz, tools/make_golden_decode.py)."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import build_llm_product, rel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gold():
    return dict(np.load(os.path.join(GOLD, "llm_decode_tiny.npz"))), json.load(open(os.path.join(GOLD, "llm_decode_meta.json")))


def _greedy():
    from cosyvoice_lora_finetune_framework_amd import utils as U
    return functools.partial(U.ras_sampling, top_k=1, tau_r=1e9)


def _tiny(dtype=torch.float32):
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    _, meta = _gold()
    m = build_llm_product(meta["tiny"], DEV, Numerics(dtype=dtype))
    m.sampling = _greedy()
    return m


# ------------------------------------------------------------------------------------------------ decode linear
LIN_SHAPES = [(1024, 1024), (1024, 3072), (4096, 1024), (1024, 4096), (1024, 4097), (128, 51)]


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K,N", LIN_SHAPES)
def test_decode_linear_vs_fp64(K, N, wdt):
    from cosyvoice_lora_finetune_framework_amd.decode import decode_linear
    g = torch.Generator(device="cpu").manual_seed(K * 7 + N)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(wdt)
    b = torch.randn(N, generator=g) * 0.1
    lg, lb = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    Wd = W.to(DEV)
    for M in (1, 3, 16):
        X = torch.randn(M, K, generator=g) * 2 + 0.5
        R = torch.randn(M, N, generator=g)
        x64, w64 = X.double(), W.double()
        xn = (x64 - x64.mean(1, keepdim=True)) / torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + 1e-5)
        xn = xn * lg.double() + lb.double()
        cases = {
            "plain": (dict(), x64 @ w64.T),
            "bias_relu_ln": (dict(bias=b.to(DEV), ln=(lg.to(DEV), lb.to(DEV), 1e-5), act=1),
                             torch.relu(xn @ w64.T + b.double())),
            "bias_residual": (dict(bias=b.to(DEV), residual=R.to(DEV)), x64 @ w64.T + b.double() + R.double()),
        }
        for name, (kw, ref) in cases.items():
            y = decode_linear(X.to(DEV), Wd, **kw)
            torch.cuda.synchronize()
            assert rel(y, ref) < 1e-5, (M, name, rel(y, ref))


def test_decode_linear_residual_in_place():
    from cosyvoice_lora_finetune_framework_amd.decode import decode_linear
    g = torch.Generator(device="cpu").manual_seed(3)
    W = torch.randn(1024, 4096, generator=g) / 64
    X, H = torch.randn(2, 4096, generator=g), torch.randn(2, 1024, generator=g)
    h = H.to(DEV).clone()
    decode_linear(X.to(DEV), W.to(DEV), residual=h, out=h)
    assert rel(h, H.double() + X.double() @ W.double().T) < 1e-5


# ------------------------------------------------------------------------------------------------ decode attention
def _attn_ref(q, kc, vc, kn, vn, P, u, v, L0, Lq):
    """fp64: one sequence, one head.  q/kn/vn [Lq, 64], kc/vc [L0, 64], P [>= L0+Lq, 64]."""
    k = torch.cat([kc[:L0], kn]).double()
    vv = torch.cat([vc[:L0], vn]).double()
    out = torch.zeros(Lq, 64, dtype=torch.float64)
    for r in range(Lq):
        i = L0 + r
        j = torch.arange(i + 1)
        s = ((q[r].double() + u.double()) @ k[:i + 1].T + (P[i - j].double() @ (q[r].double() + v.double()))) / 8.0
        out[r] = torch.softmax(s, 0) @ vv[:i + 1]
    return out


@pytest.mark.parametrize("Lq", [1, 5])
def test_decode_attn_ragged_split_append(Lq):
    from cosyvoice_lora_finetune_framework_amd.decode import decode_attn
    g = torch.Generator(device="cpu").manual_seed(11 + Lq)
    B, H, cap = 3, 16, 1536
    D = H * 64
    lens = [1, 37, 1500]
    kc, vc = torch.zeros(B, H, cap, 64), torch.zeros(B, H, cap, 64)
    for b, L in enumerate(lens):
        kc[b, :, :L] = torch.randn(H, L, 64, generator=g)
        vc[b, :, :L] = torch.randn(H, L, 64, generator=g)
    qkv = torch.randn(B * Lq, 3 * D, generator=g)
    P = torch.randn(cap, D, generator=g) * 0.5
    u, v = torch.randn(H, 64, generator=g) * 0.1, torch.randn(H, 64, generator=g) * 0.1
    for done in (None, torch.tensor([0, 1, 0], dtype=torch.int32)):
        kd, vd = kc.to(DEV), vc.to(DEV)
        o = decode_attn(qkv.to(DEV), kd, vd, torch.tensor(lens, dtype=torch.int32, device=DEV), P.to(DEV), u.to(DEV),
                        v.to(DEV), B, H, Lq, done=None if done is None else done.to(DEV)).cpu()
        kd, vd = kd.cpu(), vd.cpu()
        for b, L in enumerate(lens):
            rows = slice(b * Lq, (b + 1) * Lq)
            skipped = done is not None and bool(done[b])
            for h in range(H):
                q = qkv[rows, h * 64:(h + 1) * 64]
                kn = qkv[rows, D + h * 64:D + (h + 1) * 64]
                vn = qkv[rows, 2 * D + h * 64:2 * D + (h + 1) * 64]
                if skipped:
                    assert torch.equal(o[rows, h * 64:(h + 1) * 64], torch.zeros(Lq, 64))
                    assert torch.equal(kd[b, h], kc[b, h]) and torch.equal(vd[b, h], vc[b, h])
                    continue
                ref = _attn_ref(q, kc[b, h], vc[b, h], kn, vn, P[:, h * 64:(h + 1) * 64], u[h], v[h], L, Lq)
                assert rel(o[rows, h * 64:(h + 1) * 64], ref) < 1e-5, (b, h)
                assert torch.equal(kd[b, h, L:L + Lq], kn) and torch.equal(vd[b, h, L:L + Lq], vn)
                assert torch.equal(kd[b, h, :L], kc[b, h, :L]) and not kd[b, h, L + Lq:].any()


# ------------------------------------------------------------------------------------------------ sampler
class _State:
    def __init__(self, B, V, eos, hist_rows=None, step=1, min_len=0, max_len=1000, seeds=None):
        i32 = lambda x: torch.as_tensor(x, dtype=torch.int32).to(DEV)   # noqa: E731
        self.B, self.V, self.eos = B, V, eos
        self.tok, self.next_in, self.err, self.done = i32([0] * B), i32([0] * B), i32([0] * B), i32([0] * B)
        self.hist = torch.zeros(B, 64, dtype=torch.int32)
        self.nhist = torch.zeros(B, dtype=torch.int32)
        for b, h in enumerate(hist_rows or []):
            self.hist[b, :len(h)] = torch.tensor(h, dtype=torch.int32)
            self.nhist[b] = len(h)
        self.hist, self.nhist = self.hist.to(DEV), self.nhist.to(DEV)
        self.step, self.min_len, self.max_len = i32([step] * B), i32([min_len] * B), i32([max_len] * B)
        self.len = i32([5] * B)
        self.seeds = torch.as_tensor(seeds if seeds is not None else list(range(B)), dtype=torch.int64).to(DEV)

    def run(self, logits, mode=0, top_k=25, top_p=0.8, win=10, rep_thr=1, uniforms=None):
        from cosyvoice_lora_finetune_framework_amd.hipops.binding import check, lib, ptr, stream
        logp = torch.empty_like(logits)
        check(lib().cvft_decode_sample(self.B, self.V, ptr(logits), logits.stride(0), ptr(logp), self.eos, mode, top_k,
                                       top_p, win, rep_thr, ptr(self.seeds), ptr(uniforms), ptr(self.tok),
                                       ptr(self.next_in), ptr(self.hist), 64, ptr(self.nhist), ptr(self.step),
                                       ptr(self.min_len), ptr(self.max_len), ptr(self.len), ptr(self.done), ptr(self.err),
                                       stream()), "cvft_decode_sample")
        torch.cuda.synchronize()
        return logp


def _inv_cdf(p, u):
    c = np.cumsum(p)
    i = int(np.searchsorted(c, u * c[-1], side="right"))
    return min(i, len(p) - 1)


def _restate(probs, hist, u0, u1, top_k, top_p, win, rep_thr):
    """the reference rules on fp32 probabilities (common.py:111-139), draws by inverse CDF."""
    order = sorted(range(len(probs)), key=lambda i: (-probs[i], i))
    cand, cum = [], np.float32(0)
    for i in order:
        if cum < np.float32(top_p) and len(cand) < top_k:
            cum = np.float32(cum + probs[i])
            cand.append(i)
        else:
            break
    pick = cand[_inv_cdf(np.array([probs[i] for i in cand], dtype=np.float64), u0)]
    rep = sum(1 for t in hist[-win:] if t == pick) if win > 0 else 0
    if rep >= rep_thr:
        pick = _inv_cdf(probs.astype(np.float64), u1)
    return pick


def test_sampler_pinned_uniforms_match_the_rules():
    g = torch.Generator(device="cpu").manual_seed(5)
    B, V, eos = 16, 4097, 4096
    logits = torch.randn(B, V, generator=g) * 3
    logits[:, 100:110] = logits[:, 100:101]            # exact ties
    logits[::2, 100] = logits[::2].max(1).values + 1.0  # tied near the top on even rows
    logits[::2, 100:104] = logits[::2, 100:101]
    hists = [[int(logits[b].argmax())] * (b % 3) + [7, 9] for b in range(B)]
    U = torch.rand(B, 101, 2, generator=g)
    st = _State(B, V, eos, hists)
    logp = st.run(logits.to(DEV), uniforms=U.to(DEV))
    assert rel(logp, torch.log_softmax(logits.double(), 1)) < 1e-6
    got = st.tok.cpu().tolist()
    for b in range(B):
        probs = torch.softmax(logp[b].cpu().double(), 0).float().numpy()
        want = _restate(probs, hists[b], float(U[b, 0, 0]), float(U[b, 0, 1]), 25, 0.8, 10, 1)
        assert got[b] == want, (b, got[b], want)
    assert st.nhist.cpu().tolist() == [len(h) + 1 for h in hists]
    assert st.len.cpu().tolist() == [6] * B and st.step.cpu().tolist() == [2] * B
    assert st.next_in.cpu().tolist() == got


def test_sampler_eos_rules():
    B, V, eos = 4, 51, 50
    logits = torch.zeros(B, V)
    logits[:, eos] = 30.0                     # EOS is (by far) the argmax
    logits[:, 3] = 5.0
    # step 0: EOS masked -> greedy picks 3 even though min_len is 0
    st = _State(B, V, eos, step=0, min_len=0)
    st.run(logits.to(DEV), top_k=1, rep_thr=11)
    assert st.tok.cpu().tolist() == [3] * B and not st.done.any()
    # before min_len: EOS re-drawn 100 times, then the error flag
    st = _State(B, V, eos, step=1, min_len=5)
    st.run(logits.to(DEV), top_k=1, rep_thr=11)
    assert st.err.cpu().tolist() == [1] * B and st.done.cpu().tolist() == [1] * B
    # at / after min_len: EOS accepted and ends the row (nothing appended)
    st = _State(B, V, eos, step=5, min_len=5)
    st.run(logits.to(DEV), top_k=1, rep_thr=11)
    assert st.tok.cpu().tolist() == [eos] * B and st.done.cpu().tolist() == [1] * B and not st.err.any()
    assert st.nhist.cpu().tolist() == [0] * B and st.len.cpu().tolist() == [5] * B
    # the re-draw loop uses fresh uniforms: EOS with probability ~1/2 is re-drawn until another id comes
    logits = torch.zeros(B, V)
    logits[:, eos] = math.log(V - 1.0)
    st = _State(B, V, eos, step=1, min_len=5, seeds=[11, 12, 13, 14])
    st.run(logits.to(DEV), mode=2)
    toks = st.tok.cpu().tolist()
    assert all(t != eos for t in toks) and not st.err.any()
    # max_len ends the row after its last token
    st = _State(B, V, eos, step=9, max_len=10)
    st.run(torch.randn(B, V).to(DEV), top_k=1, rep_thr=11)
    assert st.done.cpu().tolist() == [1] * B and st.tok.cpu().tolist() != [eos] * B


def test_sampler_device_draws_follow_the_ras_mixture():
    B, V, eos = 1 << 16, 4097, 4096
    g = torch.Generator(device="cpu").manual_seed(9)
    row = torch.randn(V, generator=g) * 2.5
    hist = [int(i) for i in row.topk(3).indices[[0, 2]]] + [17]      # the window holds the 1st and 3rd most likely ids
    st = _State(B, V, eos, [hist] * B, seeds=list(range(1000, 1000 + B)))
    logits = row.to(DEV).expand(B, V).contiguous()
    logp = st.run(logits)
    probs = torch.softmax(logp[0].cpu().double(), 0).numpy()
    order = sorted(range(V), key=lambda i: (-probs[i], i))
    cand, cum = [], np.float32(0)
    for i in order:
        if cum < np.float32(0.8) and len(cand) < 25:
            cum = np.float32(cum + np.float32(probs[i]))
            cand.append(i)
        else:
            break
    pn = np.zeros(V)
    pn[cand] = probs[cand] / probs[cand].sum()
    W = set(hist)
    pW = sum(pn[t] for t in W)
    exp = np.array([pn[t] * (t not in W) for t in range(V)]) + pW * probs
    cnt = np.bincount(st.tok.cpu().numpy(), minlength=V).astype(np.float64)
    big = exp * B >= 20
    sig = np.sqrt(B * exp[big] * (1 - exp[big]))
    assert np.all(np.abs(cnt[big] - B * exp[big]) <= 5 * sig)
    rest_e, rest_c = exp[~big].sum() * B, cnt[~big].sum()
    assert abs(rest_c - rest_e) <= 5 * math.sqrt(rest_e) + 5


def test_sampler_seed_not_batch_position():
    V, eos = 4097, 4096
    g = torch.Generator(device="cpu").manual_seed(2)
    row = torch.randn(V, generator=g)
    a = _State(1, V, eos, seeds=[777])
    a.run(row.to(DEV)[None].contiguous(), top_k=50, top_p=0.95)
    b = _State(8, V, eos, seeds=[1, 2, 3, 4, 5, 777, 6, 7])
    b.run(row.to(DEV).expand(8, V).contiguous(), top_k=50, top_p=0.95)
    assert b.tok.cpu().tolist()[5] == a.tok.cpu().tolist()[0]


# ------------------------------------------------------------------------------------------------ model level
def test_forward_chunk_matches_reference():
    arr, meta = _gold()
    m = _tiny()
    n = meta["tiny"]["fc_steps"]
    cache, cnn, off = torch.zeros(0, 0, 0, 0, device=DEV), torch.zeros(0, 0, 0, 0, device=DEV), 0
    for i in range(n):
        x = torch.from_numpy(arr[f"fc_x{i}"]).to(DEV)
        T = x.shape[1]
        y, cache, cnn = m.llm.forward_chunk(x, offset=off, required_cache_size=-1, att_cache=cache, cnn_cache=cnn,
                                            att_mask=torch.tril(torch.ones(1, T, T, device=DEV)).bool())
        off += T
        assert rel(y, torch.from_numpy(arr[f"fc_y{i}"])) < 1e-4, i
        if f"fc_cache{i}" in arr:
            ref = torch.from_numpy(arr[f"fc_cache{i}"])
            assert cache.shape == ref.shape and rel(cache, ref) < 1e-4, i
    assert list(cnn.shape) == meta["tiny"]["fc_cnn_shape"]
    # required_cache_size > 0 keeps the last rows only
    _, c2, _ = m.llm.forward_chunk(torch.from_numpy(arr["fc_x0"]).to(DEV), 0, 7)
    assert c2.shape[2] == 7 and rel(c2, torch.from_numpy(arr["fc_cache0"])[:, :, -7:]) < 1e-4


def _case(arr, k):
    t = lambda n: torch.from_numpy(arr[f"{k}_{n}"])           # noqa: E731
    text, ptext, ptok, emb = t("text"), t("ptext"), t("ptok"), t("emb")
    return (text.to(DEV), torch.tensor([text.shape[1]]), ptext.to(DEV), torch.tensor([ptext.shape[1]]), ptok.to(DEV),
            torch.tensor([ptok.shape[1]]), emb.to(DEV))


@pytest.mark.parametrize("case", ["i", "ii"])
def test_inference_greedy_matches_reference(case):
    arr, _ = _gold()
    m = _tiny()
    ref = arr[f"{case}_tokens"].tolist()
    lp = arr[f"{case}_lp"]
    toks, dev_lp = [], []
    for t in m.inference(*_case(arr, case)):
        toks.append(t)
        sess = next(iter(m._cvft_sessions.values()))[1]
        dev_lp.append(sess.logp[0].cpu())
    assert toks == ref
    assert m.speech_token_size not in toks
    n_text = arr[f"{case}_text"].shape[1]
    assert len(toks) == int(n_text * 20) == len(ref)          # these cases run to max_len
    d = (torch.stack(dev_lp).double() - torch.from_numpy(lp[:len(dev_lp)]).double()).abs()
    assert float((d / torch.from_numpy(lp[:len(dev_lp)]).double().abs().clamp_min(1.0)).max()) <= 1e-4


def test_inference_eos_before_min_len_raises():
    arr, meta = _gold()
    m = _tiny()
    with torch.no_grad():
        m.llm_decoder.bias[m.speech_token_size] += meta["tiny"]["eos_bias_bump"]
    with pytest.raises(RuntimeError) as e:
        list(m.inference(*_case(arr, "iii")))
    assert str(e.value) == meta["tiny"]["error"]


def test_inference_host_callable_matches_device_sampler():
    arr, _ = _gold()
    m = _tiny()
    ref = arr["ii_tokens"].tolist()
    m.sampling = lambda s, d, n: s.argmax().reshape(1)        # any callable: drawn on the host per step
    assert list(m.inference(*_case(arr, "ii"))) == ref


def test_graph_decode_bit_identical_to_eager():
    arr, _ = _gold()
    m = _tiny()
    m.sampling = None                                          # ras defaults, device draws
    args = _case(arr, "i")
    runs = []
    for use_graph in (True, False):
        toks = []
        for t in m.inference(*args, seed=1234, use_graph=use_graph, min_token_text_ratio=20):
            toks.append(t)
            if len(toks) == 64:
                sess = next(iter(m._cvft_sessions.values()))[1]
                runs.append((toks, sess.logits.cpu().clone()))
                break
    assert len(runs) == 2 and len(runs[0][0]) == 64
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    torch.manual_seed(5)
    a = list(m.inference(*args))
    torch.manual_seed(5)
    assert list(m.inference(*args)) == a


@pytest.mark.parametrize("sampled", [False, True])
def test_inference_batch_equals_single_runs(sampled):
    m = _tiny()
    if sampled:
        m.sampling = None
    g = torch.Generator(device="cpu").manual_seed(77)
    texts = [torch.randint(0, 100, (n,), generator=g) for n in (4, 2, 3, 1)]
    embs = [torch.zeros(1, 192), torch.randn(1, 192, generator=g), torch.zeros(0, 192), torch.randn(1, 192, generator=g)]
    seeds = [101, 202, 303, 404]
    batch = m.inference_batch([t.to(DEV) for t in texts], embeddings=[e.to(DEV) for e in embs], seeds=seeds,
                              min_token_text_ratio=0.5)
    for b in range(4):
        z = torch.zeros(1, 0, dtype=torch.long, device=DEV)
        one = list(m.inference(texts[b][None].to(DEV), torch.tensor([texts[b].numel()]), z, torch.tensor([0]), z,
                               torch.tensor([0]), embs[b].to(DEV), min_token_text_ratio=0.5, seed=seeds[b]))
        assert batch[b] == one, b


def test_full_size_fp32_tokens_and_bf16_teacher_forced():
    from cosyvoice_lora_finetune_framework_amd.decode import SamplerCfg
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    meta = json.load(open(os.path.join(GOLD, "llm_decode_meta.json")))["full"]
    ref = dict(np.load(os.path.join(GOLD, "llm_decode_full.npz")))
    m = build_llm_product(meta, DEV, Numerics(), full=True)
    m.sampling = _greedy()
    text = torch.from_numpy(ref["text"]).to(DEV)
    z = torch.zeros(1, 0, dtype=torch.long, device=DEV)
    args = (text, torch.tensor([text.shape[1]]), z, torch.tensor([0]), z, torch.tensor([0]), torch.zeros(1, 192, device=DEV))
    toks, lp_tok, top8, lse = [], [], [], []
    for t in m.inference(*args, max_token_text_ratio=0.8, min_token_text_ratio=0.0):
        sess = next(iter(m._cvft_sessions.values()))[1]
        toks.append(t)
        lp = sess.logp[0].double().cpu()
        lp_tok.append(float(lp[t]))
        top8.append(lp.topk(8).values)
        lse.append(float(sess.logits[0].double().logsumexp(0)))
    assert toks == ref["tokens"].tolist()
    # per-step log-probabilities of the fp32 path: logp[token], the top-8 values, the logsumexp of the raw logits
    assert np.abs(np.array(lp_tok) - ref["logp_tok"]).max() <= 1e-4
    assert np.abs(torch.stack(top8).numpy() - ref["top8"]).max() <= 1e-4
    assert np.abs((np.array(lse) - ref["lse"]) / np.maximum(np.abs(ref["lse"]), 1.0)).max() <= 1e-4
    # bf16 weights: feed the reference tokens, compare logp[token] per step
    m.numerics = Numerics(dtype=torch.bfloat16)
    rows, _ = m.lm_input_rows(*args)
    sess = m.decode_session(1, rows.shape[0] + 32)
    sess.start([rows], [0], [32], [0], SamplerCfg("logp"))
    got = []
    for i, t in enumerate(ref["tokens"].tolist()):
        got.append(float(sess.logp[0, t]))
        sess.next_in.fill_(t)
        sess.advance()
        sess.stack.len.add_(1)
    err = np.abs(np.array(got) - ref["logp_tok"])
    print("bf16 |dlogp| max", err.max(), "mean", err.mean())
    assert err.max() <= 0.05           # measured 5.3e-3 max, 1.5e-3 mean


def _joint_models():
    from helpers import build_flow_product
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    meta = json.load(open(os.path.join(GOLD, "tiny_meta.json")))
    return _tiny(), build_flow_product(meta["flow"], DEV, Numerics()), meta


def test_joint_synthesize_matches_reference():
    """greedy LLM tokens -> flow.inference (noise pinned) -> de-normalised mel, against the reference's joint path
    (tests/golden/llm_decode_joint.npz), also at speed 0.8."""
    from cosyvoice_lora_finetune_framework_amd.inference_joint import synthesize
    arr, _ = _gold()
    ref = dict(np.load(os.path.join(GOLD, "llm_decode_joint.npz")))
    llm, flow, _ = _joint_models()
    z = torch.from_numpy(ref["z"]).to(DEV)
    text = arr["i_text"][0].tolist()
    tokens, mel = synthesize(llm, flow, text, noise=z)
    assert tokens == ref["tokens"][0].tolist()
    want = torch.from_numpy(ref["mel"])
    assert tuple(mel.shape) == tuple(want.shape) and rel(mel, want) < 1e-4, rel(mel, want)
    _, slow = synthesize(llm, flow, text, speed=0.8, noise=z)
    want = torch.from_numpy(ref["mel_speed08"])
    assert tuple(slow.shape) == tuple(want.shape) and rel(slow, want) < 1e-4, rel(slow, want)


def test_joint_cli_writes_the_reference_mel(tmp_path):
    from cosyvoice_lora_finetune_framework_amd.inference_joint import main
    from cosyvoice_lora_finetune_framework_amd.lora import get_merged_state_dict
    arr, _ = _gold()
    ref = dict(np.load(os.path.join(GOLD, "llm_decode_joint.npz")))
    llm, flow, meta = _joint_models()
    torch.save({k: v.cpu() for k, v in get_merged_state_dict(llm).items()}, tmp_path / "llm.pt")
    torch.save({k: v.cpu() for k, v in get_merged_state_dict(flow).items()}, tmp_path / "flow.pt")
    np.save(tmp_path / "z.npy", ref["z"])
    c = meta["llm"]["build"]
    llm_cfg = dict(text_encoder_input_size=c["text_in"], llm_input_size=c["d"], llm_output_size=c["d"],
                   text_token_size=c["text_vocab"], speech_token_size=c["speech_vocab"], attention_heads=c["heads"],
                   linear_units=c["ff"], text_encoder_blocks=c["text_blocks"], llm_blocks=c["llm_blocks"])
    out = tmp_path / "mel.npy"
    main(["--llm", str(tmp_path / "llm.pt"), "--flow", str(tmp_path / "flow.pt"),
          "--text-tokens", ",".join(str(int(t)) for t in arr["i_text"][0]), "--out", str(out), "--top-k", "1",
          "--tau-r", "1e9", "--llm-config", json.dumps(llm_cfg), "--flow-config", json.dumps(meta["flow"]["build"]),
          "--noise", str(tmp_path / "z.npy"), "--speed", "0.8"])
    mel = np.load(out)
    assert mel.shape == ref["mel_speed08"].shape[1:]
    assert rel(torch.from_numpy(mel), torch.from_numpy(ref["mel_speed08"][0])) < 1e-4


def test_sessions_share_packed_weights_and_stay_bounded():
    m = _tiny()
    s = [m.decode_session(1, 256 * (i + 1)) for i in range(m.MAX_SESSIONS + 2)]
    assert len(m._cvft_sessions) == m.MAX_SESSIONS
    assert all(x.stack.layers is s[0].stack.layers and x.W_dec is s[0].W_dec for x in s)
    assert m.decode_session(1, 256 * (m.MAX_SESSIONS + 2)) is s[-1]


def test_pinned_uniforms_are_not_captured_by_address():
    arr, _ = _gold()
    m = _tiny()
    m.sampling = None
    args = _case(arr, "i")
    g = torch.Generator(device="cpu").manual_seed(8)
    U1, U2 = torch.rand(1, 101, 2, generator=g).to(DEV), torch.rand(1, 101, 2, generator=g).to(DEV)
    a1 = list(m.inference(*args, uniforms=U1, min_token_text_ratio=20))
    a2 = list(m.inference(*args, uniforms=U2, min_token_text_ratio=20))
    e2 = list(m.inference(*args, uniforms=U2, min_token_text_ratio=20, use_graph=False))
    assert a2 == e2 and a1 != a2
