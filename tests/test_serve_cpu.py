"""Continuous batching, the host-only part (decode.RowScheduler / prefill_chunks / serve_schedule): which request takes
which cache row, in which chunks its prompt is prefilled and when its first token is due.  No GPU."""
import pytest

from cosyvoice_lora_finetune_framework_amd import decode as D


@pytest.mark.parametrize("prefill_rows", [0, 1, 6, 15])
@pytest.mark.parametrize("T", [1, 5, 6, 7, 16, 17, 43, 300])
def test_chunks_cover_the_prompt_and_respect_the_limit(T, prefill_rows):
    chunks = D.prefill_chunks(T, prefill_rows)
    assert sum(chunks) == T and min(chunks) >= 1
    assert max(chunks) <= (prefill_rows if prefill_rows else D.MAX_ROWS)
    assert all(c == (prefill_rows or D.MAX_ROWS) for c in chunks[:-1])          # only the last chunk is short


@pytest.mark.parametrize("rows,prefill_rows", [(8, 9), (16, 1), (1, 16), (0, 0), (17, 0), (4, -1)])
def test_more_than_16_activation_rows_are_refused(rows, prefill_rows):
    with pytest.raises(ValueError):
        D.RowScheduler(rows, prefill_rows)
    with pytest.raises(ValueError):
        D.check_serve_rows(rows, prefill_rows)


def test_limits_that_fit_are_taken():
    for rows, n in [(16, 0), (8, 8), (1, 15), (10, 6)]:
        D.RowScheduler(rows, n)


REQS = [(0, 7, 12), (0, 43, 60), (0, 5, 6), (4, 20, 30), (11, 4, 3)]        # (arrival step, prompt rows, tokens)


@pytest.mark.parametrize("prefill_rows", [0, 6])
def test_admission_is_fifo_one_at_a_time_and_rows_are_reused(prefill_rows):
    sch = D.serve_schedule(2, prefill_rows, REQS)
    admits = [s["admit_step"] for s in sch]
    assert admits == sorted(admits) and len(set(admits)) == len(admits)          # arrival order, one admission per step
    for (arrival, T, n), s in zip(REQS, sch):
        assert s["admit_step"] >= arrival
        assert [c for _, c in s["chunks"]] == D.prefill_chunks(T, prefill_rows)
        steps = [st for st, _ in s["chunks"]]
        if prefill_rows == 0:
            assert set(steps) == {s["admit_step"]}                               # stall: the whole prompt in the admission's step
        else:
            assert steps == list(range(s["admit_step"], s["admit_step"] + len(steps)))       # one chunk per step, no gap
        assert s["first_step"] == steps[-1]                                      # first token with the last prompt row
        assert s["last_step"] == s["first_step"] + n - 1                         # then one token per step
    # one admission in flight: a request's first chunk comes after the previous request's last
    for a, b in zip(sch, sch[1:]):
        assert b["chunks"][0][0] > a["chunks"][-1][0]
    # two rows: requests 0 and 1 take rows 0 and 1; the long request 1 keeps its row while the short ones share the other
    assert [s["row"] for s in sch[:2]] == [0, 1]
    assert sch[2]["row"] == sch[0]["row"] and sch[2]["admit_step"] > sch[0]["last_step"]
    # never two requests in one row at a time
    for i, a in enumerate(sch):
        for b in sch[i + 1:]:
            if a["row"] == b["row"]:
                assert b["admit_step"] > a["last_step"]


def test_a_freed_row_goes_to_the_oldest_queued_request_and_cancel_leaves_the_queue():
    s = D.RowScheduler(2, 4)
    for rid, T in enumerate([9, 3, 5, 2]):
        s.submit(rid, T)
    p = s.plan()
    assert p["admit"] == (0, 0) and p["chunks"] == [4] and not p["first"]
    assert s.plan()["admit"] is None                                             # request 0 is still being prefilled
    p = s.plan()
    assert p["chunks"] == [1] and p["first"] and p["rid"] == 0
    p = s.plan()
    assert p["admit"] == (1, 1) and p["chunks"] == [3] and p["first"]
    p = s.plan()                                                                 # both rows taken: nothing to admit
    assert p == dict(admit=None, rid=None, row=None, chunks=[], first=False)
    assert s.release(3) is None and [q for q, _ in s.queue] == [2]               # a queued request is cancelled
    assert s.release(0) == 0
    p = s.plan()
    assert p["admit"] == (2, 0) and p["chunks"] == [4]
    assert s.release(2) == 0 and s.flight is None                                # cancelled while it is being prefilled
    assert s.release(1) == 1 and not s.busy() and s.free == [0, 1]


def test_stall_mode_uses_all_sixteen_rows():
    sch = D.serve_schedule(16, 0, [(0, 300, 40)] * 16)
    assert sorted(s["row"] for s in sch) == list(range(16))
    assert all(max(c for _, c in s["chunks"]) == 16 and len(s["chunks"]) == 19 for s in sch)
