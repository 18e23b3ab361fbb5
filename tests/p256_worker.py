"""fp64 restatement of cvft_gemm's 256x256 kernel (csrc/gemm_p256.hip) and the checks tests/test_gemm_p256_gpu.py runs on it.

The test imports this module for its in-process cases (default knobs).  It also starts it as a child process for the forms
that only a knob selects: gemm_p256.hip and gemm_glds.hip read their CVFT_* knobs into statics on the first launch, so
every knob set needs a fresh process.  As a child:  python p256_worker.py CASES.json OUT.json  runs every case of the list
in order and writes one metrics record per case; the parent asserts on them.

Reference:  C = epi(alpha * (A W^T + ext) + bias), the chain in the order of p256_epilogue_rows / gemm_epilogue_direct8
(gemm_common.h): preact, act, act'(dact_src), output dropout, residual.  ext = U Bl^T, or with xdrop the sum over the
16-wide rank tiles t of mask_t / (1 - p) * U_t Bl_t^T.  Operands are bf16; the reference takes the same stored values to
fp64.  Masks come from the host replica of the device mask (tests/helpers.py)."""
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "tests"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

from helpers import keep_scale_host  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
TILE = 256
GUARD_ROWS, GUARD_COLS = 8, 32      # sentinel rows above / below and columns left / right of the output views (32 bf16 = 64 B)
SENTINEL = 1232.0                   # (exact in bf16)
ODROP_SITE = 29

ACT = {None: lambda t: t, "relu": Fn.relu, "silu": Fn.silu, "gelu_erf": Fn.gelu,
       "gelu_tanh": lambda t: Fn.gelu(t, approximate="tanh")}


def _dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def _dgelu_erf(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


DACT = {"relu": lambda x: (x > 0).double(), "silu": _dsilu, "gelu_erf": _dgelu_erf}


def HF():
    from cosyvoice_lora_finetune_framework_amd.hipops import functional as F
    return F


def case(name, M, N, K, **kw):
    """One launch form.  ext: None | "plain" | "xdrop" (R % 16 == 0, one mask site per rank tile); strided: A, W, U, Bl,
    dact_src, residual, C and preact are views into wider buffers (C keeps ldc == N under output dropout, as the ABI needs);
    hints: the cvft_set_concurrent_chains values to run under (None = leave it); p256_rows: the rows the 256x256 kernel
    computes itself (the rest is the row split's 128-row remainder launch) -- rows that must be bit-identical across hints."""
    c = dict(name=name, M=M, N=N, K=K, R=0, ext=None, sites=None, pdrop=0.15, bias=False, alpha=1.0, act=None, preact=False,
             dact=None, odrop=0.0, residual=False, strided=True, wzero=False, seed=1, splitk=False, hints=[None], p256_rows=M,
             kind="check")
    c.update(kw)
    if c["R"] and c["ext"] is None:
        c["ext"] = "plain"
    if c["ext"] == "xdrop" and c["sites"] is None:
        c["sites"] = [11 + t for t in range(c["R"] // 16)]
    return c


class Out:
    """An output view into a buffer filled with SENTINEL: GUARD_ROWS rows above and below it, GUARD_COLS columns on either
    side when `cols` (ldc > N).  poison() fills the view with NaN before a launch; guard_ok() checks every element outside
    the view bit for bit."""

    def __init__(self, M, N, cols):
        gc = GUARD_COLS if cols else 0
        self.buf = torch.full((M + 2 * GUARD_ROWS, N + 2 * gc), SENTINEL, dtype=BF, device=DEV)
        self.view = self.buf[GUARD_ROWS:GUARD_ROWS + M, gc:gc + N]
        self.box = (GUARD_ROWS, GUARD_ROWS + M, gc, gc + N)
        self.init = self.buf.clone()

    def poison(self):
        self.view.fill_(float("nan"))

    def guard_ok(self):
        d = self.buf.view(torch.int16) != self.init.view(torch.int16)
        r0, r1, c0, c1 = self.box
        d[r0:r1, c0:c1] = False
        return not bool(d.any())


def _in(data, strided):
    """`data` as a view into a buffer GUARD_COLS columns wider on each side, filled with NaN there (ld > columns): a kernel
    that reads past a row end poisons its outputs"""
    if not strided:
        return data.contiguous()
    r, c = data.shape
    buf = torch.full((r, c + 2 * GUARD_COLS), float("nan"), dtype=data.dtype, device=DEV)
    v = buf[:, GUARD_COLS:GUARD_COLS + c]
    v.copy_(data)
    return v


def make_ops(c, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    M, N, K, R, st = c["M"], c["N"], c["K"], c["R"], c["strided"]
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device=DEV) * scale).to(BF)       # noqa: E731
    o = {"A": _in(rn(M, K), st)}
    o["W"] = _in(torch.zeros(N, K, dtype=BF, device=DEV) if c["wzero"] else rn(N, K, scale=1 / math.sqrt(K)), st)
    o["U"] = _in(rn(M, R), st) if R else None
    o["Bl"] = _in(rn(N, R, scale=0.5 / math.sqrt(R)), st) if R else None       # the rank term: ~1/4 of the output variance
    o["bias"] = torch.randn(N, generator=g, device=DEV) * 0.5 if c["bias"] else None
    o["dact_src"] = _in(rn(M, N), st) if c["dact"] else None
    o["residual"] = _in(rn(M, N), st) if c["residual"] else None
    o["C"] = Out(M, N, st and not c["odrop"])
    o["P"] = Out(M, N, st) if c["preact"] else None
    return o


def launch(c, o, poison=True):
    """one cvft_gemm launch of case c on the current stream; returns the kernel label"""
    F = HF()
    if poison:
        o["C"].poison()
        if o["P"] is not None:
            o["P"].poison()
    kw = {}
    if c["R"]:
        kw.update(U=o["U"], Bl=o["Bl"])
    if c["ext"] == "xdrop":
        kw["xdrop"] = (c["pdrop"], list(c["sites"]))
    if c["odrop"]:
        kw["odrop"] = (c["odrop"], ODROP_SITE)
    F.gemm(o["A"], o["W"], bias=o["bias"], alpha=c["alpha"], act=c["act"], preact=None if o["P"] is None else o["P"].view,
           dact_src=o["dact_src"], dact=c["dact"], residual=o["residual"], out=o["C"].view, **kw)
    return F.lib().cvft_gemm_last_kernel().decode()


def seed_now():
    F = HF()
    F.dropout_begin_step()
    return int(F._DROPOUT["seed"].item())


def mask(seed, site, p, M, N):
    return keep_scale_host(seed, site, M * N, p).view(M, N).to(DEV)


def reference(c, o, seed):
    """(pre-activation, output) in fp64"""
    M, N = c["M"], c["N"]
    d = lambda t: t.double()        # noqa: E731
    z = d(o["A"]) @ d(o["W"]).t()
    if c["ext"] == "plain":
        z += d(o["U"]) @ d(o["Bl"]).t()
    elif c["ext"] == "xdrop":
        for t, site in enumerate(c["sites"]):
            s = slice(16 * t, 16 * t + 16)
            z += mask(seed, site, c["pdrop"], M, N) * (d(o["U"][:, s]) @ d(o["Bl"][:, s]).t())
    z *= float(torch.tensor(c["alpha"], dtype=torch.float32))
    if o["bias"] is not None:
        z += d(o["bias"])
    v = ACT[c["act"]](z)
    if c["dact"]:
        v = v * DACT[c["dact"]](d(o["dact_src"]))
    if c["odrop"]:
        v = v * mask(seed, ODROP_SITE, c["odrop"], M, N)
    if o["residual"] is not None:
        v = v + d(o["residual"])
    return z, v


def errors(got, ref):
    """(max relative L2 error over the 256x256 output tiles, over the rows, whole tensor) of bf16 `got` against fp64 `ref`"""
    M, N = ref.shape
    e2 = (got.double() - ref).square_()
    r2 = ref.square()
    tm = (M + TILE - 1) // TILE

    def tiles(x):
        pad = torch.zeros((tm * TILE, N), dtype=x.dtype, device=x.device)
        pad[:M] = x
        return pad.view(tm, TILE, N // TILE, TILE).sum((1, 3))
    tile = float((tiles(e2) / tiles(r2).clamp_min(1e-300)).sqrt().max())
    row = float((e2.sum(1) / r2.sum(1).clamp_min(1e-300)).sqrt().max())
    whole = float((e2.sum() / r2.sum().clamp_min(1e-300)).sqrt())
    return tile, row, whole


def measure(c, o, pre_ref, ref, label):
    """metrics record of the launch whose results are in o"""
    C, P = o["C"], o["P"]
    r = {"label": label, "nan": bool(torch.isnan(C.view).any()), "guard": C.guard_ok()}
    r["tile"], r["row"], r["whole"] = errors(C.view, ref)
    if P is not None:
        r["nan"] = r["nan"] or bool(torch.isnan(P.view).any())
        r["guard"] = r["guard"] and P.guard_ok()
        r["pre_tile"], r["pre_row"], _ = errors(P.view, pre_ref)
    return r


def bits(t):
    return t.contiguous().view(torch.int16).clone()


def run_check(c):
    """The launch under every chains hint of c["hints"] (each against fp64), then the last hint once more: rows
    [0, p256_rows) bit-identical across hints, the repeat bit-identical to its first run."""
    lib = HF().lib()
    seed = seed_now()
    o = make_ops(c, c["seed"])
    pre_ref, ref = reference(c, o, seed)
    rec = {"name": c["name"], "runs": []}
    outs = []
    old = lib.cvft_concurrent_chains()
    try:
        for h in list(c["hints"]) + [c["hints"][-1]]:
            if h is not None:
                lib.cvft_set_concurrent_chains(h)
            label = launch(c, o)
            torch.cuda.synchronize()
            rec["runs"].append(dict(measure(c, o, pre_ref, ref, label), hint=h))
            outs.append([bits(o["C"].view)] + ([bits(o["P"].view)] if o["P"] is not None else []))
    finally:
        lib.cvft_set_concurrent_chains(old)
    m1 = c["p256_rows"]
    rec["repeat_same"] = all(torch.equal(a, b) for a, b in zip(outs[-1], outs[-2]))
    rec["hints_same"] = all(torch.equal(a[:m1], b[:m1]) for k in range(1, len(outs) - 1) for a, b in zip(outs[0], outs[k]))
    return rec


def run_mask(c):
    """Exact mask placement: W = 0 and no bias, so a dropped output is exactly 0.  xdrop with one rank tile: C = mask * U Bl^T;
    output dropout: C = mask * (U Bl^T).  Where |U Bl^T| > 1e-3 the zero pattern of C must equal the host mask element for
    element, under every hint (both remainder tiles of the row split)."""
    assert c["wzero"] and not c["bias"] and not c["residual"] and c["act"] is None and c["R"] == 16 and c["alpha"] == 1.0
    lib = HF().lib()
    seed = seed_now()
    o = make_ops(c, c["seed"])
    M, N = c["M"], c["N"]
    site, p = (c["sites"][0], c["pdrop"]) if c["ext"] == "xdrop" else (ODROP_SITE, c["odrop"])
    keep = mask(seed, site, p, M, N) > 0
    big = (o["U"].double() @ o["Bl"].double().t()).abs() > 1e-3
    rec = {"name": c["name"], "runs": []}
    old = lib.cvft_concurrent_chains()
    try:
        for h in c["hints"]:
            if h is not None:
                lib.cvft_set_concurrent_chains(h)
            label = launch(c, o)
            torch.cuda.synchronize()
            kept = o["C"].view != 0
            bad = (kept != keep) & big
            rows = bad.any(1).nonzero().flatten()
            rec["runs"].append({"label": label, "hint": h, "nan": bool(torch.isnan(o["C"].view).any()), "guard": o["C"].guard_ok(),
                                "mismatch": int(bad.sum()), "bad_rows": [int(rows.min()), int(rows.max())] if len(rows) else [],
                                "compared": int(big.sum()), "compared_in_remainder": int(big[c["p256_rows"]:].sum()),
                                "keep_rate": float(kept[big].float().mean())})
    finally:
        lib.cvft_set_concurrent_chains(old)
    return rec


_STREAMS = []


def _streams():
    """the two side streams and the capture stream of run_splitk, the same for every case of the process: the split-K
    workspace pool hands every stream it sees a slot of its own and holds 8"""
    if not _STREAMS:
        _STREAMS.extend(torch.cuda.Stream() for _ in range(3))
    return _STREAMS


def run_splitk(c):
    """Split-K (CVFT_P256_SPLIT): the launch twice (arrival tickets back at zero: both right, bit-identical); two launches
    on two streams at once with different operands (one workspace slot each: both right); eager, then a single-stream
    graph capture and replay (the workspace was grown eagerly): the replay bit-identical to eager."""
    seed = seed_now()
    o = make_ops(c, c["seed"])
    pre_ref, ref = reference(c, o, seed)
    rec = {"name": c["name"], "runs": []}
    rec["runs"].append(dict(measure(c, o, pre_ref, ref, launch(c, o)), form="eager"))
    torch.cuda.synchronize()
    first = bits(o["C"].view)
    rec["runs"].append(dict(measure(c, o, pre_ref, ref, launch(c, o)), form="again"))
    torch.cuda.synchronize()
    rec["repeat_same"] = torch.equal(first, bits(o["C"].view))
    # two streams
    o2 = make_ops(c, c["seed"] + 100)
    pre_ref2, ref2 = reference(c, o2, seed)
    o["C"].poison()
    o2["C"].poison()
    cur = torch.cuda.current_stream()
    s1, s2, cap = _streams()
    s1.wait_stream(cur)
    s2.wait_stream(cur)
    with torch.cuda.stream(s1):
        l1 = launch(c, o, poison=False)
    with torch.cuda.stream(s2):
        l2 = launch(c, o2, poison=False)
    cur.wait_stream(s1)
    cur.wait_stream(s2)
    torch.cuda.synchronize()
    rec["runs"].append(dict(measure(c, o, pre_ref, ref, l1), form="stream1"))
    rec["runs"].append(dict(measure(c, o2, pre_ref2, ref2, l2), form="stream2"))
    rec["stream_same"] = torch.equal(first, bits(o["C"].view))
    # graph capture and replay
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        lg = launch(c, o, poison=False)
    o["C"].poison()
    g.replay()
    torch.cuda.synchronize()
    rec["runs"].append(dict(measure(c, o, pre_ref, ref, lg), form="graph"))
    rec["graph_same"] = torch.equal(first, bits(o["C"].view))
    del g
    return rec


RUN = {"check": run_check, "mask": run_mask, "splitk": run_splitk}


def run(c):
    return RUN[c["kind"]](c)


def main():
    with open(sys.argv[1]) as f:
        cases = json.load(f)
    torch.cuda.set_device(0)
    out = []
    for c in cases:
        out.append(run(c))
        print(c["name"], "ok", flush=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
