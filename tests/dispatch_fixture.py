"""Shared by tests/test_gemm_dispatch_cpu.py and tests/test_gemm_dispatch_gpu.py: the recorded dispatch table
(tests/golden/gemm_dispatch.json, tools/make_golden_dispatch.py) and cvft_gemm_plan, the query that names what cvft_gemm
would launch without a GPU.

The library reads its CVFT_* knobs once per process, so the non-default knob sets of the fixture are replayed by a child:
    python dispatch_fixture.py SET_INDEX OUT.json
replays every entry of that set under its knobs and writes the list of results."""
import contextlib
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
FIXTURE = os.path.join(REPO, "tests", "golden", "gemm_dispatch.json")
OPERANDS = ("in_len", "out_len", "A", "W", "U", "Bl", "bias", "preact", "dact_src", "residual", "C", "La", "Uout", "xdrop_seed")


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def plan_text(lib, args):
    """(rc, text of cvft_gemm_plan) for a GemmArgs"""
    buf = C.create_string_buffer(512)
    rc = lib.cvft_gemm_plan(C.byref(args), buf, len(buf))
    return rc, buf.value.decode()


def plan_lines(text):
    """[(label, first row, row count)] of a plan text"""
    out = []
    for line in text.splitlines():
        label, rest = line.split(" grid=")
        r0, n = rest.split("rows=")[1].split("+")
        out.append((label, int(r0), int(n)))
    return out


def fake_args(sig):
    """cvft_gemm_args of a fixture signature: operands are addresses nobody owns, 64 GiB apart, of the recorded alignment"""
    from cosyvoice_lora_finetune_framework_amd.hipops.binding import GemmArgs
    g = GemmArgs()
    for k, v in sig["args"].items():
        if isinstance(v, list):
            for i, x in enumerate(v):
                getattr(g, k)[i] = x
        else:
            setattr(g, k, v)
    g.alpha = g.lora_scale = 1.0
    for name, off in sig["ptr"].items():
        setattr(g, name, ((OPERANDS.index(name) + 1) << 36) + off)
    return g


def replay(lib, entries, hints):
    """what cvft_gemm_plan says for every entry under every hint, in the form the fixture records: [rc, label or error]"""
    out = []
    old = lib.cvft_concurrent_chains()
    try:
        for e in entries:
            g, res = fake_args(e), {}
            for h in hints:
                lib.cvft_set_concurrent_chains(h)
                rc, text = plan_text(lib, g)
                res[str(h)] = [rc, plan_lines(text)[-1][0] if rc == 0 else lib.cvft_last_error().decode()]
            out.append(res)
    finally:
        lib.cvft_set_concurrent_chains(old)
    return out


def expected(e):
    """The recorded result of an entry.  One kind of entry carries "since_plan": launches whose row-split remainder the
    LDS-DMA kernels do not take were an error when the fixture was recorded ("res" keeps that record) and are the single
    unsplit 256x256 launch since the selection plans before it enqueues."""
    if "since_plan" in e:
        assert all(rc == -1 and text.startswith("cvft_gemm: row split:") for rc, text in e["res"].values()), e
        return e["since_plan"]
    return e["res"]


@contextlib.contextmanager
def planned(lib):
    """Inside the block every cvft_gemm first asks cvft_gemm_plan about the same arguments; yields the list of (rc, text)."""
    real, seen = lib.cvft_gemm, []

    def both(aref, st):
        seen.append(plan_text(lib, aref._obj))
        return real(aref, st)

    lib.cvft_gemm = both
    try:
        yield seen
    finally:
        lib.cvft_gemm = real


def main():
    doc = load()
    s = doc["sets"][int(sys.argv[1])]
    os.environ.update(s["knobs"])
    import torch  # noqa: F401
    from cosyvoice_lora_finetune_framework_amd.hipops import binding as cb
    with open(sys.argv[2], "w") as f:
        json.dump(replay(cb.lib(), s["entries"], doc["hints"]), f)


if __name__ == "__main__":
    main()
