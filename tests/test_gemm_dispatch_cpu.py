"""cvft_gemm's dispatch table without a GPU: for every signature, chains hint and knob set recorded in
tests/golden/gemm_dispatch.json (tools/make_golden_dispatch.py: real launches, observed through cvft_gemm_last_kernel /
cvft_last_error) cvft_gemm_plan must give the same return code and name the same kernel, or the same error."""
import json
import os
import subprocess
import sys

import torch  # noqa: F401  (bind to torch's HIP runtime first)

import dispatch_fixture as DF

HERE = os.path.dirname(os.path.abspath(__file__))


def _lib():
    from cosyvoice_lora_finetune_framework_amd.hipops import binding as cb
    if not os.path.exists(cb.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return cb.lib()


def _mismatches(knobs, entries, got):
    assert len(got) == len(entries)
    return [(knobs, e["args"], e["ptr"], h, want, g[h]) for e, g in zip(entries, got) for h, want in DF.expected(e).items() if g[h] != want]


def test_fixture_holds_the_cases():
    doc = DF.load()
    assert doc["hints"] == [1, 3]
    knobs = [s["knobs"] for s in doc["sets"]]
    assert knobs[0] == {}
    for k in ({"CVFT_P256": "0"}, {"CVFT_P256": "2"}, {"CVFT_P256_ROWSPLIT": "0"}, {"CVFT_P256_SPLIT": "3"}, {"CVFT_P256_NARROW": "84"},
              {"CVFT_GLDS_WIDE": "0"}, {"CVFT_GLDS_WIDE": "1"}, {"CVFT_GLDS_CFG": "-1"}, {"CVFT_GLDS_DIRECT": "0"}):
        assert k in knobs
    default = doc["sets"][0]["entries"]
    assert sum(e.get("src") == "bench" for e in default) >= 100 and sum("src" not in e for e in default) >= 150
    assert all(set(e["res"]) == {"1", "3"} for s in doc["sets"] for e in s["entries"])


def test_default_knobs_plan_what_was_launched():
    doc = DF.load()
    s = doc["sets"][0]
    assert not any(k.startswith(("CVFT_GLDS_", "CVFT_P256", "CVFT_SKINNY_MT")) for k in os.environ)
    bad = _mismatches({}, s["entries"], DF.replay(_lib(), s["entries"], doc["hints"]))
    assert not bad, (len(bad), bad[:5])


def test_knob_sets_plan_what_was_launched(tmp_path):
    doc = DF.load()
    _lib()
    env = {k: v for k, v in os.environ.items() if not k.startswith(("CVFT_GLDS_", "CVFT_P256", "CVFT_SKINNY_MT"))}
    kids = [(i, subprocess.Popen([sys.executable, os.path.join(HERE, "dispatch_fixture.py"), str(i), str(tmp_path / f"{i}.json")], env=env))
            for i in range(1, len(doc["sets"]))]
    bad = []
    for i, kid in kids:
        assert kid.wait(timeout=300) == 0, doc["sets"][i]["knobs"]
        with open(tmp_path / f"{i}.json") as f:
            bad += _mismatches(doc["sets"][i]["knobs"], doc["sets"][i]["entries"], json.load(f))
    assert len(kids) >= 9
    assert not bad, (len(bad), bad[:5])
