"""cvft_gemm's 256x256 kernel (csrc/gemm_p256.hip) in every form it launches, against an fp64 restatement of the same
operation on the same bf16 operands (tests/p256_worker.py).

Every case asserts the gemm_p256_kernel label (",xdrop" / ",splitk" where expected), the maximum relative L2 error over the
256x256 output tiles and over the rows (one wrong tile or row group fails, not only the whole tensor), that no NaN of the
poisoned outputs is left, and that the sentinel rows and columns around the strided output views are untouched.

In process, default knobs: the three in-step launches of the LLM (w_2 dgrad, w_1 forward, stacked q|k|v forward) at M = 5328
and a second layout, under the full grid and the half-width multi-item grid of the joint step; the plain rank extension as
an extra k-tile; the masked rank extension; partial last row tiles; exact mask placement across the row split.
Knob-only forms run in a child process each (the knobs are read once per process): CVFT_P256=2 edge sweep, split-K with
fp32 and bf16 slabs, CVFT_P256_ROWSPLIT=0, CVFT_P256_GRID, CVFT_P256_NARROW.

Tolerances (relative L2, per tile and per row).  The error is the bf16 rounding of the output on an fp32 accumulation: on an
MI355X at most 1.9e-3 per tile and 2.2e-3 per row (the 256-column rows of the edge sweep) over every fp32-accumulated case;
TOL is about 2x that.  Split-K with bf16 slabs rounds every k-split's partial tile to bf16 once more before the fp32 sum, a
second rounding of the same size as the output's: at most 2.4e-3 per tile and 2.9e-3 per row, so TOL_SLAB_BF16 is 1.4x TOL."""
import json
import os
import subprocess
import sys

import pytest

import p256_worker as PW
from p256_worker import case

pytestmark = pytest.mark.gpu

TOL = 4e-3
TOL_SLAB_BF16 = 5.5e-3
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "p256_worker.py")


def split_rows(M, N):
    """rows the 256x256 kernel computes itself under default knobs: gemm_p256_plan's row split (256 < tiles <= 416)
    hands the tile rows behind the first 256 / tiles_n to a 128-row remainder launch"""
    tm, tn = -(-M // 256), N // 256
    if 256 < tm * tn <= 416 and 1 <= 256 // tn < tm:
        return (256 // tn) * 256
    return M


def instep(name, M, N, K, **kw):
    return case(name, M, N, K, hints=[1, 3], p256_rows=split_rows(M, N), **kw)


# the in-step signatures (profiles/r4_insitu_gemm_table.txt): w_2 dgrad in train mode (act'(h) of the ReLU, the producer's
# keep scale as alpha, masked LoRA extension), w_1 forward (bias, act, inner dropout, LoRA extension), q|k|v forward (bias,
# stacked rank-48 extension); each at M = 5328 and a second layout: 7000 x 4096 (448 tiles, no row split, several rounds),
# 4100 x 4096 (row split, a 4-row remainder), 7000 x 3072 (row split at row 5376).  silu / gelu_erf: ReLU commutes with the
# non-negative dropout scale, so only these see the order of act and output dropout.
INSTEP = [
    instep("w2_dgrad", 5328, 4096, 1024, R=16, ext="xdrop", sites=[5], dact="relu", alpha=1 / 0.9),
    instep("w2_dgrad", 7000, 4096, 1024, R=16, ext="xdrop", sites=[5], dact="relu", alpha=1 / 0.9),
    instep("w2_dgrad_silu", 5328, 4096, 1024, R=16, ext="xdrop", sites=[6], dact="silu", odrop=0.1),
    instep("w1_fwd", 5328, 4096, 1024, R=16, bias=True, act="relu", odrop=0.1),
    instep("w1_fwd", 4100, 4096, 1024, R=16, bias=True, act="relu", odrop=0.1),
    instep("w1_fwd_silu", 5328, 4096, 1024, R=16, bias=True, act="silu", preact=True, odrop=0.1),
    instep("w1_fwd_gelu", 4100, 4096, 1024, R=16, bias=True, act="gelu_erf", preact=True, odrop=0.1, residual=True),
    instep("qkv_fwd", 5328, 3072, 1024, R=48, bias=True),
    instep("qkv_fwd", 7000, 3072, 1024, R=48, bias=True, alpha=0.75),
]
# plain rank extension as one more k-tile of the pipeline, R % 16 != 0 included (chunks >= R masked in registers); 192 tiles
PLAIN = [case(f"plain_r{r}", 4096, 3072, 1024, R=r, bias=True, act="gelu_tanh", preact=True, residual=True) for r in (8, 24, 40, 64)]
# masked rank extension with a distinct mask site per 16-wide rank tile
XDROP = [case(f"xdrop_r{r}", 4096, 3072, 1024, R=r, ext="xdrop", residual=True, alpha=0.5) for r in (16, 32, 64)]
# partial last row tiles (208 rows; 1 row) at the smallest auto k-loop and a long one
PARTIAL = [
    case("partial_5328_k512", 5328, 3072, 512, bias=True, act="silu", preact=True, residual=True),
    case("partial_5328_k4096", 5328, 3072, 4096, R=16, dact="gelu_erf", residual=True, alpha=0.5),
    case("partial_2049_k512", 2049, 6144, 512, R=32, ext="xdrop", bias=True, odrop=0.1),
    case("partial_2049_k4096", 2049, 6144, 4096, bias=True, act="relu", preact=True, residual=True),
]


def check(rec, c, tol=TOL):
    """assert every run of a worker record (see p256_worker.run_check / run_splitk / run_mask)"""
    for r in rec["runs"]:
        where = (c["name"], c["M"], c["N"], c["K"], r.get("hint"), r.get("form"))
        lab = r["label"]
        assert lab.startswith("gemm_p256_kernel"), (where, lab)
        assert (",xdrop" in lab) == (c["ext"] == "xdrop"), (where, lab)
        assert (",splitk" in lab) == c["splitk"], (where, lab)
        assert not r["nan"], (where, "NaN left in a poisoned output")
        assert r["guard"], (where, "sentinel around an output view overwritten")
        if "tile" in r:
            assert r["tile"] < tol and r["row"] < tol, (where, f"max rel error per tile {r['tile']:.3e}, per row {r['row']:.3e}, tol {tol}")
        if "pre_tile" in r:
            assert r["pre_tile"] < tol and r["pre_row"] < tol, (where, f"preact: per tile {r['pre_tile']:.3e}, per row {r['pre_row']:.3e}")
    for k in ("repeat_same", "hints_same", "stream_same", "graph_same"):
        if k in rec:
            assert rec[k], (c["name"], c["M"], k)
    print(json.dumps({"case": c["name"], "M": c["M"], "K": c["K"], "R": c["R"],
                      "tile": max((r.get("tile", 0) for r in rec["runs"]), default=0),
                      "row": max((r.get("row", 0) for r in rec["runs"]), default=0),
                      "pre": max((r.get("pre_row", 0) for r in rec["runs"]), default=0)}))


@pytest.mark.parametrize("c", INSTEP + PLAIN + XDROP + PARTIAL, ids=lambda c: f"{c['name']}-{c['M']}x{c['N']}x{c['K']}")
def test_p256_matches_fp64(c):
    """one launch form against fp64; in-step forms also under chains hint 1 (full grid) and 3 (half-width grid, several
    items per workgroup): the rows the 256x256 kernel computes bit-identical, the row split's remainder (96x256 or 128x128
    tiles by hint) against fp64 only; a repeated launch bit-identical"""
    check(PW.run(c), c)


@pytest.mark.parametrize("c", [
    case("mask_xdrop", 5328, 4096, 1024, R=16, ext="xdrop", wzero=True, kind="mask", hints=[1, 3], p256_rows=4096),
    case("mask_odrop", 5328, 4096, 1024, R=16, odrop=0.1, wzero=True, kind="mask", hints=[1, 3], p256_rows=4096),
], ids=lambda c: c["name"])
def test_p256_mask_placement_across_row_split(c):
    """5328 x 4096 splits at row 4096: the masked rank extension's and the output dropout's keep patterns equal the host mask
    element for element on both sides of the split (row_off of the remainder launch), under both remainder tiles"""
    assert split_rows(c["M"], c["N"]) == c["p256_rows"]
    rec = PW.run(c)
    check(rec, c)
    for r in rec["runs"]:
        assert r["compared"] > 0.9 * c["M"] * c["N"] and r["compared_in_remainder"] > 0, r
        assert r["mismatch"] == 0, (c["name"], r)
        p = c["pdrop"] if c["ext"] == "xdrop" else c["odrop"]
        assert abs(r["keep_rate"] - (1 - p)) < 5e-3, r


# ---------------------------------------------------------------- knob-only forms: one child process per knob set

def _worker(tmp_path, knobs, cases, timeout=300):
    """run the cases in a fresh process under exactly these CVFT_P256* knobs; fails (never retries) on a non-zero exit or a
    timeout, with the child's output -- and ends the session after a timeout or a crash, which may have left the GPU faulted"""
    env = {k: v for k, v in os.environ.items() if not k.startswith(("CVFT_P256", "CVFT_GLDS"))}
    env.update({k: str(v) for k, v in knobs.items()})
    cj, oj = tmp_path / "cases.json", tmp_path / "out.json"
    cj.write_text(json.dumps(cases))
    try:
        r = subprocess.run([sys.executable, WORKER, str(cj), str(oj)], env=env, timeout=timeout, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        out = e.output.decode(errors="replace") if isinstance(e.output, bytes) else (e.output or "")
        pytest.exit(f"p256 worker {knobs} timed out after {timeout} s (a hang: nothing more runs on this GPU):\n{out[-8000:]}", 1)
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit(f"p256 worker {knobs} died with {r.returncode} (nothing more runs on this GPU):\n{r.stdout[-8000:]}", 1)
    if r.returncode != 0:
        pytest.fail(f"p256 worker {knobs} exited with {r.returncode}:\n{r.stdout[-8000:]}")
    recs = json.loads(oj.read_text())
    assert [x["name"] for x in recs] == [c["name"] for c in cases]
    return recs


def _edge_cases():
    """N = 256 (one tile column), M in {1, 255, 257, 300}, k-loops of 1 .. 7 k-tiles, with and without the rank extension
    (the extension k-tile behind a single k-tile included), the masked extension on a few"""
    out = []
    for K in (64, 128, 192, 320, 448):
        for i, M in enumerate((1, 255, 257, 300)):
            epi = [dict(bias=True, act="silu", preact=True), dict(residual=True, alpha=0.5), dict(dact="gelu_erf", bias=True),
                   dict(act="relu", residual=True, preact=True)][i]
            out.append(case(f"edge_{M}x256x{K}", M, 256, K, **epi))
            out.append(case(f"edge_{M}x256x{K}_r16", M, 256, K, R=16, **epi))
        out.append(case(f"edge_257x256x{K}_r24", 257, 256, K, R=24, bias=True))
        out.append(case(f"edge_257x256x{K}_xdrop32", 257, 256, K, R=32, ext="xdrop", residual=True))
    return out


def test_p256_edge_sweep_forced(tmp_path):
    """CVFT_P256=2: the kernel whenever legal -- single tile column, 1 .. 300 rows, k-loops of 1 .. 7 k-tiles"""
    cases = _edge_cases()
    for rec, c in zip(_worker(tmp_path, {"CVFT_P256": 2}, cases), cases):
        check(rec, c)


def _split_cases():
    out = []
    for K in (1024, 4096):        # 84 tiles; 16 / 64 k-tiles (5 splits: an uneven deal)
        out.append(case(f"split_plain_k{K}", 5328, 1024, K, kind="splitk", splitk=True, bias=True, act="silu", preact=True))
        out.append(case(f"split_r16_k{K}", 5328, 1024, K, R=16, kind="splitk", splitk=True, bias=True, residual=True))
        out.append(case(f"split_xdrop_k{K}", 5328, 1024, K, R=32, ext="xdrop", kind="splitk", splitk=True, dact="relu",
                        odrop=0.1, alpha=1 / 0.9))
    return out


@pytest.mark.parametrize("slab_bf16", [0, 1])
@pytest.mark.parametrize("S", [2, 3, 5])
def test_p256_split_k(tmp_path, S, slab_bf16):
    """CVFT_P256_SPLIT (CVFT_P256=2: the auto mode would also want tiles x S >= 192): plain, rank-16 extension and masked
    extension; a second launch (the arrival tickets are back at zero), two streams at once (one workspace slot each) and a
    graph replay (workspace grown eagerly) -- all right, the repeat, the first stream and the replay bit-identical to eager"""
    cases = _split_cases()
    recs = _worker(tmp_path, {"CVFT_P256": 2, "CVFT_P256_SPLIT": S, "CVFT_P256_SLAB_BF16": slab_bf16}, cases)
    for rec, c in zip(recs, cases):
        check(rec, c, TOL_SLAB_BF16 if slab_bf16 else TOL)


def test_p256_no_row_split(tmp_path):
    """CVFT_P256_ROWSPLIT=0 at 5328 x 4096: all 336 tiles in one launch, more than one round (and a multi-item grid)"""
    cases = [case("norowsplit_w2_dgrad", 5328, 4096, 1024, R=16, ext="xdrop", dact="relu", alpha=1 / 0.9, hints=[1, 3]),
             case("norowsplit_w1_fwd", 5328, 4096, 1024, R=16, bias=True, act="silu", preact=True, odrop=0.1, hints=[1, 3])]
    for rec, c in zip(_worker(tmp_path, {"CVFT_P256_ROWSPLIT": 0}, cases), cases):
        check(rec, c)


@pytest.mark.parametrize("grid", [24, 40])
def test_p256_capped_grid(tmp_path, grid):
    """CVFT_P256_GRID=24 / 40: uneven rounds of items per workgroup"""
    cases = [case(f"grid{grid}_qkv", 5328, 3072, 1024, R=48, bias=True),
             case(f"grid{grid}_w2_dgrad", 5328, 4096, 1024, R=16, ext="xdrop", dact="relu", alpha=1 / 0.9, p256_rows=4096),
             case(f"grid{grid}_w1_fwd", 7000, 4096, 1024, R=16, bias=True, act="gelu_erf", odrop=0.1)]
    for rec, c in zip(_worker(tmp_path, {"CVFT_P256_GRID": grid}, cases), cases):
        check(rec, c)


def test_p256_narrow(tmp_path):
    """CVFT_P256_NARROW=64: the N = 1024 LLM launches (84 tiles) on the 256x256 kernel"""
    cases = []
    for K in (1024, 4096):
        cases.append(case(f"narrow_fwd_k{K}", 5328, 1024, K, R=16, bias=True, residual=True, odrop=0.1))
        cases.append(case(f"narrow_dgrad_k{K}", 5328, 1024, K, R=16, ext="xdrop", residual=True))
    for rec, c in zip(_worker(tmp_path, {"CVFT_P256_NARROW": 64}, cases), cases):
        check(rec, c)
