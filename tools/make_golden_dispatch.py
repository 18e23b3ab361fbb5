#!/usr/bin/env python3
"""Golden record of cvft_gemm's dispatch table (tests/golden/gemm_dispatch.json).

For a list of argument signatures the tool launches cvft_gemm on uninitialised buffers of the right extents and records
what came back: the return code plus cvft_gemm_last_kernel(), or cvft_last_error().  Every signature runs under the
chains hints 1 and 3 (cvft_set_concurrent_chains).  tests/test_gemm_dispatch_cpu.py replays the record through
cvft_gemm_plan without a GPU.  Only cvft_gemm, cvft_gemm_last_kernel, cvft_set_concurrent_chains and cvft_last_error are
used, so the tool runs unchanged on a commit that predates cvft_gemm_plan (that is how the record was made).

The library reads its CVFT_* knobs once per process, so one invocation records ONE knob set:

  python tools/make_golden_dispatch.py --collect SIGS.json
        one step of bench.py's default joint configuration with the binding's cvft_gemm wrapped: every distinct
        signature functional.gemm and the fused / conv callers issue
  python tools/make_golden_dispatch.py --signatures SIGS.json
        default knobs: the collected signatures (a) and the threshold probes (b)
  python tools/make_golden_dispatch.py --set CVFT_P256=0          (one call per entry of KNOB_SETS)
        a knob set (c): the probes tagged for knob sets

Each call replaces its own section of --out (default tests/golden/gemm_dispatch.json) and keeps the others.

A signature is {"args": non-zero integer / float fields of cvft_gemm_args, "ptr": {operand: byte offset from a 16-byte
boundary}} -- operands missing from "ptr" are NULL.  Fields left out are zero.

The committed record was made on the commit before cvft_gemm planned its launches.  One entry of it (CVFT_GLDS_DIRECT=0, masked
rank extension on the row-split shape) recorded the error that commit returned when the row split's remainder was not
eligible; it carries a hand-written "since_plan" beside "res": the single unsplit 256x256 launch that is planned since.
A fresh recording has that result in "res" itself.
"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

OUT = os.path.join(REPO, "tests", "golden", "gemm_dispatch.json")
HINTS = (1, 3)
KNOB_SETS = ["CVFT_P256=0", "CVFT_P256=2", "CVFT_P256_ROWSPLIT=0", "CVFT_P256_SPLIT=3", "CVFT_P256_SPLIT=-1", "CVFT_P256_NARROW=84",
             "CVFT_GLDS_WIDE=0", "CVFT_GLDS_WIDE=1", "CVFT_GLDS_CFG=-1", "CVFT_GLDS_DIRECT=0"]
POINTERS = ("in_len", "out_len", "A", "W", "U", "Bl", "bias", "preact", "dact_src", "residual", "C", "La", "Uout", "xdrop_seed")
SKIP = ("alpha", "lora_scale")          # never looked at by the selection


# ------------------------------------------------------------------------------------ signatures
def sig(M, N, K, dtype=1, R=0, fuse=False, taps=(0,), geo=None, flags="", off=None, **kw):
    """One signature.  flags: b bias, p preact, d dact_src, r residual, i in_len, o out_len; R with fuse = La / Uout, else
    U / Bl; geo = (Tm, Tin, Tout, in_stride, out_stride, out_off); off = {operand: misalignment in bytes}; kw overrides
    any cvft_gemm_args field (leading dimensions default to the tight ones)."""
    Tm, Tin, Tout, ins, outs, outo = geo or (M, M, M, 1, 1, 0)
    a = dict(dtype=dtype, M=M, N=N, K=K, Tm=Tm, Tin=Tin, Tout=Tout, in_stride=ins, out_stride=outs, out_off=outo,
             ntaps=len(taps), tap_off=list(taps) + [0] * (4 - len(taps)), lda=K, ldw=len(taps) * K, ldc=N)
    ptr = dict(A=0, W=0, C=0)
    if R:
        a.update(R=R, ldbl=R, ldu=R)
        ptr["Bl"] = 0
        if fuse:
            a["ldla"] = K
            ptr.update(La=0, Uout=0)
        else:
            ptr["U"] = 0
    for f, name, ld in (("b", "bias", None), ("p", "preact", "ldp"), ("d", "dact_src", "ldd"), ("r", "residual", "ldr"),
                        ("i", "in_len", None), ("o", "out_len", None)):
        if f in flags:
            ptr[name] = 0
            if ld:
                a[ld] = N
    if "d" in flags:
        a["dact"] = 2
    if kw.get("xdrop_p") or kw.get("odrop_p"):
        ptr["xdrop_seed"] = 0
    if kw.get("xdrop_p") and "xdrop_sites" not in kw:
        a["xdrop_sites"] = [11, 12, 13, 14]
    a.update(kw)
    ptr.update(off or {})
    return {"args": {k: v for k, v in a.items() if v not in (0, 0.0, [0, 0, 0, 0])}, "ptr": {k: v for k, v in ptr.items() if v is not None}}


def probes():
    """(signature, in_knob_sets) pairs: one step either side of every threshold of the selection rules"""
    P, G = (5328, 4096, 1024), (2048, 1024, 256)        # the 256x256 kernel's home shape (row split) / an LDS-DMA 64x64 shape
    out = []
    add = lambda s, knobs=False: out.append((s, knobs))       # noqa: E731
    # N 32 / 33 and 64 / 65; skinny's N % 16 and its epilogue-free condition
    for N in (16, 32, 33, 48, 56, 64, 65, 80):
        add(sig(512, N, 256), knobs=N == 32)
        add(sig(512, N, 256, flags="b"))
    for M in (4096, 4097):                               # skinny rows per block
        add(sig(M, 48, 1536))
    # K % 64 and K % 32 (and K % 8: vector loads)
    for K in (256, 224, 208, 100, 32, 24):
        add(sig(512, 32, K))
        add(sig(2048, 1024, K), knobs=K == 224)
    # t64 around big_thr = 1000, with a short and a deep k-loop
    for M, N in ((2368, 1728), (2560, 1600)):
        for K in (256, 512):
            add(sig(M, N, K), knobs=K == 512)
    # blocks at 512 / 513 and 768 / 769: small tiles, then 128x64 tiles
    for M, N in ((2048, 1024), (1728, 1216), (2048, 1536), (49216, 64), (4096, 1024), (3456, 1216)):
        add(sig(M, N, 256, flags="b"))
    # nk at 3 / 4 and 7 / 8 (stage count; 128x128 and 256x256), 11 / 12 (k-splits)
    for K in (192, 256, 448, 512):
        add(sig(2048, 512, K))
        add(sig(2560, 1600, K))
        add(sig(2048, 6144, K))
    for K in (448, 512, 704, 768):
        add(sig(5328, 1024, K), knobs=True)
    # 256x256: M 2047 / 2048, tiles 191 / 192, row split at tiles 256 / 257 and 416 / 417, the smallest shape that splits
    for M in (2047, 2048):
        add(sig(M, 6144, 512), knobs=M == 2048)
    for M in (48896, 48897, 65536, 65537, 106496, 106497):
        add(sig(M, 256, 512))
    add(sig(2048, 5888, 512))
    add(sig(2304, 8192, 512), knobs=True)
    add(sig(35584, 768, 512))
    for s in (P, (5328, 1024, 4096), (5328, 3072, 1024)):
        add(sig(*s), knobs=True)
    add(sig(*P, flags="bpdr"), knobs=True)
    add(sig(*P, flags="o"))
    add(sig(4096, 4096, 1024, geo=(1024, 1024, 1024, 1, 1, 0)))
    add(sig(5328, 4224, 1024), knobs=True)                                      # N % 256 != 0: 128x128 with the XCD rectangles
    add(sig(128, 4224, 1024))                                                   # too few tile rows for the rectangles
    add(sig(*P, off={"C": 8}))
    add(sig(*P, off={"C": 4}))
    add(sig(*P, flags="b", off={"bias": 4}))
    add(sig(*P, ldc=4100))
    # the 96x256 one-round bound
    for M in (6144, 6145):
        add(sig(M, 1024, 1024), knobs=M == 6144)
    add(sig(6144, 192, 1024))
    # rank extension R on an LDS-DMA shape and on the 256x256 shape; xdrop
    for R in (8, 12, 16, 17, 48, 64, 72):
        add(sig(*G, R=R), knobs=R == 16)
        add(sig(*P, R=R), knobs=R == 16)
    for R in (16, 32, 64):
        add(sig(*G, R=R, xdrop_p=0.15), knobs=R == 16)
        add(sig(*P, R=R, xdrop_p=0.15), knobs=R == 16)
    add(sig(*G, R=8, xdrop_p=0.15))
    add(sig(*G, R=80, xdrop_p=0.15))
    add(sig(2048, 1022, 256, R=16, xdrop_p=0.15))
    add(sig(2048, 1024, 224, R=16, xdrop_p=0.15))
    add(sig(2048, 64, 256, R=16, xdrop_p=0.15))
    add(sig(*G, R=16, xdrop_p=0.15, off={"U": 8}))
    add(sig(*G, R=16, xdrop_p=1e-6))
    add(sig(*G, R=16, fuse=True, xdrop_p=0.15))
    # output dropout: every kernel honours it; its argument rule
    for s in (G, P, (2048, 1024, 224), (512, 32, 256)):
        add(sig(*s, flags="r", odrop_p=0.1, odrop_site=29), knobs=s == P)
    add(sig(*G, odrop_p=0.1, ldc=1032))
    # fused side path: R 16 / 17 / 48, with and without the LDS-DMA kernel under it
    for R in (8, 16, 17, 24, 32, 48, 49):
        add(sig(*G, R=R, fuse=True, ldbl=(R + 7) // 8 * 8), knobs=R in (16, 48))
        add(sig(2048, 1024, 224, R=R, fuse=True, ldbl=(R + 7) // 8 * 8))
    add(sig(4096, 1024, 256, R=16, fuse=True))
    add(sig(4096, 1024, 256, R=48, fuse=True))
    add(sig(*G, R=16, fuse=True, geo=(1024, 1024, 1024, 1, 1, 0)))
    add(sig(2048, 32, 256, R=16, fuse=True))
    add(sig(*G, R=16, fuse=True, off={"La": 8}))
    add(sig(512, 256, 128, dtype=0, R=4, fuse=True))
    for M, N in ((2048, 2048), (1920, 2176)):           # t128 256 / 255 under a long unpipelined K
        for K in (2080, 2016):
            add(sig(M, N, K, R=16, fuse=True))
    # unaligned A, W, U, Bl
    for name in ("A", "W", "U", "Bl"):
        add(sig(*G, R=16, off={name: 8}))
        add(sig(*P, R=16, off={name: 2}))
    add(sig(*G, lda=260))
    add(sig(*G, ldw=264))
    # register-staged kernel: ntaps * K around 2048 with t128 255 / 256
    for M, N in ((2048, 2048), (1920, 2176)):
        for K in (1024, 1016):
            add(sig(M, N, K, taps=(0, 1)))
    add(sig(4096, 512, 256, taps=(-1, 0, 1), geo=(1024, 1024, 1024, 1, 1, 0), flags="bio"))
    add(sig(2048, 512, 256, taps=(0, 1, 2), geo=(512, 1024, 512, 2, 1, 0), flags="b"))
    add(sig(2048, 512, 256, taps=(0, 1), geo=(512, 512, 1024, 1, 2, 1), flags="b"))
    add(sig(*G, flags="i"))
    add(sig(*G, flags="o"))
    add(sig(*G, flags="bpdr"), knobs=True)
    # fp32
    for s in ((512, 256, 128), (512, 32, 128), (512, 256, 130), (2048, 2048, 2048)):
        add(sig(*s, dtype=0))
    add(sig(512, 256, 128, dtype=0, R=4))
    add(sig(512, 256, 128, dtype=0, R=6))
    # argument checks
    add(sig(*G, lda=128))
    add(sig(*G, Tm=1000))
    add(sig(*G, R=49, fuse=True))
    add(sig(*G, ntaps=5))
    add(sig(*G, dtype=2))
    add(sig(*G, R=16, geo=(2048, 2048, 2048, 2, 1, 0)))
    add(sig(*G, off={"W": None}))
    return out


# ------------------------------------------------------------------------------------ launching
def fill(sg, alloc):
    """cvft_gemm_args of a signature; alloc(name, nbytes, offset) -> address of the operand (None for NULL)"""
    from cosyvoice_lora_finetune_framework_amd.hipops.binding import GemmArgs
    g = GemmArgs()
    for k, v in sg["args"].items():
        if isinstance(v, list):
            for i, x in enumerate(v):
                getattr(g, k)[i] = x
        else:
            setattr(g, k, v)
    g.alpha = g.lora_scale = 1.0
    es = 2 if g.dtype == 1 else 4
    nb = g.M // g.Tm if g.Tm > 0 else 0
    rows_out = nb * g.Tout
    need = {"A": nb * g.Tin * g.lda * es, "W": g.N * g.ldw * es, "U": g.M * g.ldu * es, "Bl": g.N * g.ldbl * es, "bias": g.N * 4,
            "preact": rows_out * g.ldp * es, "dact_src": rows_out * g.ldd * es, "residual": rows_out * g.ldr * es,
            "C": rows_out * g.ldc * es, "La": g.R * g.ldla * es, "Uout": g.M * g.ldu * es, "in_len": nb * 4, "out_len": nb * 4,
            "xdrop_seed": 8}
    for name, off in sg["ptr"].items():
        setattr(g, name, alloc(name, max(need[name], 0), off))
    return g


def record(lib, sigs):
    """launch every signature under both hints; returns the fixture entries"""
    import torch
    entries = []
    for sg in sigs:
        keep = []

        def alloc(name, nbytes, off):
            t = torch.empty(nbytes + 4096, dtype=torch.uint8, device="cuda")
            if name in ("in_len", "out_len", "xdrop_seed"):
                t.zero_()
            keep.append(t)
            return t.data_ptr() + off

        g = fill(sg, alloc)
        res = {}
        for h in HINTS:
            lib.cvft_set_concurrent_chains(h)
            rc = lib.cvft_gemm(C.byref(g), None)
            res[str(h)] = [rc, (lib.cvft_gemm_last_kernel() if rc == 0 else lib.cvft_last_error()).decode()]
        torch.cuda.synchronize()
        entries.append(dict(sg, res=res))
    lib.cvft_set_concurrent_chains(1)
    return entries


def collect(path):
    """one bench.py step (default joint configuration) with the binding's cvft_gemm wrapped"""
    import runpy
    import torch  # noqa: F401
    from cosyvoice_lora_finetune_framework_amd.hipops import binding as cb
    lib = cb.lib()
    real, seen = lib.cvft_gemm, {}

    def wrapped(aref, st):
        g = aref._obj
        args, ptr = {}, {}
        for name, _ in cb.GemmArgs._fields_:
            v = getattr(g, name)
            if name in SKIP:
                continue
            if name in POINTERS:
                if v:
                    ptr[name] = v & 15
                continue
            if not isinstance(v, (int, float)):
                v = list(v)
            if v not in (0, 0.0, [0, 0, 0, 0]):
                args[name] = v
        sg = {"args": args, "ptr": ptr}
        seen.setdefault(json.dumps(sg, sort_keys=True), sg)
        return real(aref, st)

    lib.cvft_gemm = wrapped
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "1"]
    try:
        runpy.run_path(os.path.join(REPO, "bench.py"), run_name="__main__")
    except SystemExit as e:
        assert not e.code, e.code
    lib.cvft_gemm = real
    with open(path, "w") as f:
        json.dump(list(seen.values()), f)
    print(f"{len(seen)} distinct cvft_gemm signatures -> {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--collect", metavar="FILE")
    ap.add_argument("--signatures", metavar="FILE", help="collected signatures (default knobs only; else those already in --out are kept)")
    ap.add_argument("--set", default="", help="knob set of this process, e.g. CVFT_P256=0 (several: separate by commas)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.collect:
        return collect(a.collect)
    knobs = dict(kv.split("=", 1) for kv in a.set.split(",") if kv)
    os.environ.update(knobs)
    import torch  # noqa: F401
    from cosyvoice_lora_finetune_framework_amd.hipops import binding as cb
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {"hints": list(HINTS), "sets": []}
    old = next((s for s in doc["sets"] if s["knobs"] == knobs), None)
    sigs = []
    if not knobs:
        if a.signatures:
            sigs = [dict(s, src="bench") for s in json.load(open(a.signatures))]
        elif old:
            sigs = [{k: e[k] for k in ("args", "ptr", "src")} for e in old["entries"] if e.get("src") == "bench"]
    sigs += [s for s, in_knob_sets in probes() if in_knob_sets or not knobs]
    entries = record(cb.lib(), sigs)
    doc["sets"] = [s for s in doc["sets"] if s["knobs"] != knobs] + [{"knobs": knobs, "entries": entries}]
    with open(a.out, "w") as f:
        f.write('{"hints": %s, "sets": [\n' % json.dumps(doc["hints"]))
        for i, s in enumerate(doc["sets"]):
            f.write(' {"knobs": %s, "entries": [\n  ' % json.dumps(s["knobs"]))
            f.write(",\n  ".join(json.dumps(e, sort_keys=True) for e in s["entries"]))
            f.write("\n ]}%s\n" % ("," if i + 1 < len(doc["sets"]) else ""))
        f.write("]}\n")
    print(f"[{a.set or 'default knobs'}] {len(entries)} signatures x {len(HINTS)} hints -> {a.out}")


if __name__ == "__main__":
    main()
