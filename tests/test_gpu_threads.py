"""GPU: the threading contract of the C ABI (include/gpmi355.h "Conventions") and the handle-lifetime guard (csrc/engine.hpp Guard), driven
from two to four host threads.  The scenarios live in tests/thread_cases.py and run in CHILD processes, one per group, one at a time: every context is created
there, so a host deadlock costs one time limit and can never hang this process; this process creates no context beyond the default one the autouse fixture
touches.  One test per scenario: it asserts the scenario's `ok` and prints its worst error / bound ratio, the number of overlapping call pairs and its seconds.

If a child times out, is ended by a signal or prints a HIP error text, nothing further is started: every remaining test fails at once, and nothing is retried
(the last test of this file checks that on a stand-in for the child; it needs no device, every other test here is marked `gpu`).
tests/test_abi_guard_static.py is the static side of the same contract."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GROUP_OF = {s: g for g in ("AB", "CDE", "FG", "HI") for s in g}
# seconds.  Measured once on one MI355X (profiles/r14/threads.log), serial pass + threaded pass + child start-up: AB 3.5 - 4.0 s, CDE 1.7 - 1.9 s, FG 0.9 - 1.1 s, HI 1.1 - 1.3 s
# over three runs.  Four times that is 16 / 8 / 5 / 6 s; a limit is never set below 20 s, because about a second of every figure is start-up (interpreter, NumPy / SciPy, the HIP runtime loading
# the code object) that this test does not control on a cold or busy box — a host deadlock still costs no more than 20 s.
TIMEOUT = {"AB": 20, "CDE": 20, "FG": 20, "HI": 20}
HIP_ERROR_TEXTS = ("HIP error", "hipError", "illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "core dumped")

_results = {}        # group -> {scenario: parsed JSON line}
_latch = []          # non-empty: a child ended abnormally — no further child is started


def _run_group(group):
    if group in _results:
        return _results[group]
    if _latch:
        pytest.fail(f"earlier child ended abnormally: {_latch[0]}")
    try:
        p = subprocess.run([sys.executable, "-m", "tests.thread_cases", group], timeout=TIMEOUT[group], cwd=ROOT, capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        _latch.append(f"group {group} did not finish within {TIMEOUT[group]} s (a host deadlock?); output so far: {str(e.stdout)[-600:]}")
        pytest.fail(_latch[0])
    text = p.stdout + "\n" + p.stderr
    hip = next((t for t in HIP_ERROR_TEXTS if t in text), None)
    if p.returncode != 0 or hip:  # a signal (negative, or 134 / 139 / 137 / 124 through a shell), an exception outside every scenario, or a HIP error text
        _latch.append(f"group {group}: return code {p.returncode}" + (f", HIP error text {hip!r}" if hip else "") + f"; tail of its output: {text[-800:]}")
        pytest.fail(_latch[0])
    _results[group] = {}
    for ln in p.stdout.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            _results[group][d["name"]] = d
    return _results[group]


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", list("ABCDEFGHI"))
def test_scenario(scenario):
    """A: two contexts, two threads — B: four contexts (fp64, fp32, VFE, composite), four threads — C: one context, two threads — D: handles fitted on one thread,
    used / updated / freed on another, gpd_sync and gp_get_timings in between — E: gp_logpdf_batch / _sum from two threads and gp_logpdf from a third on one
    context — F: gp_last_error() per thread — G: the process-wide "kmat_rows" toggled under a working thread — H: gp_ctx_destroy / gp_posterior_free / gp_vfe_free
    under a thread that uses the handle (each once) — I: a two-virtual-rank context created and used off the main thread."""
    lines = _run_group(GROUP_OF[scenario])
    assert scenario in lines, f"the child of group {GROUP_OF[scenario]} printed no line for scenario {scenario} (it reported {sorted(lines)})"
    d = lines[scenario]
    print(f"THREADS {scenario}: worst ratio {d['worst_ratio']}, overlapping call pairs {d['overlap_pairs']}, {d['seconds']} s; {json.dumps(d['quantities'])}"
          + "".join(f"; {k} {json.dumps(v)}" for k, v in d.items() if k not in ("name", "ok", "quantities", "worst_ratio", "overlap_pairs", "seconds", "failures")))
    assert d["ok"], f"scenario {scenario}: " + " | ".join(d["failures"])
    if scenario in "ABCDEGI":
        assert d["overlap_pairs"] > 0, "no two calls of different threads overlapped"


@pytest.mark.parametrize("how", ["signal", "abort_code", "timeout", "hip_error_text"])
def test_an_abnormal_child_stops_everything_that_follows(monkeypatch, how):
    """CPU: the stop-on-trouble rule itself, with subprocess.run replaced by a stand-in — after a child that was killed, timed out or printed a HIP error text no
    further child is started and every later request fails at once; a healthy group is started once however often it is asked for."""
    me = sys.modules[__name__]
    monkeypatch.setattr(me, "_results", {})
    monkeypatch.setattr(me, "_latch", [])
    started = []
    good = "\n".join(json.dumps({"name": n, "ok": True}) for n in "AB")

    def fake_run(cmd, timeout, **kw):
        started.append(cmd[-1])
        if cmd[-1] == "AB":
            return subprocess.CompletedProcess(cmd, 0, good, "")
        if how == "timeout":
            raise subprocess.TimeoutExpired(cmd, timeout, output="")
        out = json.dumps({"name": "C", "ok": False, "failures": ["status -1700: HIP error 700 (an illegal memory access was encountered)"]})
        return subprocess.CompletedProcess(cmd, {"signal": -11, "abort_code": 134}.get(how, 0), out if how == "hip_error_text" else "", "")

    monkeypatch.setattr(subprocess, "run", fake_run)
    assert set(_run_group("AB")) == {"A", "B"} and set(_run_group("AB")) == {"A", "B"}
    with pytest.raises(pytest.fail.Exception, match="group CDE"):
        _run_group("CDE")
    for g in ("CDE", "FG", "HI"):
        with pytest.raises(pytest.fail.Exception, match="earlier child ended abnormally"):
            _run_group(g)
    assert started == ["AB", "CDE"]
    assert set(_run_group("AB")) == {"A", "B"}  # what had finished before stays readable
