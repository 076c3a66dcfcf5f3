"""bench.py's host side, no device: what a plain run and --full select, that --steps is the number
of timed calls whatever the queue length, and the --dump-outputs files."""
import argparse
import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "1")
    assert (a.steps, a.warmup, a.pods, a.full) == (7, 1, 1_000_000, False)
    assert not a.tree and a.cpu_sample == 0 and a.c4_pods == 0 and a.per_pod_calls == 0
    a = _parse(monkeypatch, "--workload", "c2x", "--per-pod-calls", "50", "--cpu-sample", "100")
    assert a.per_pod_calls == 0 and a.cpu_sample == 0


def test_full_keeps_the_side_lines(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.tree and a.cpu_sample == 30000 and a.c4_pods == 20000 and a.per_pod_calls == 200
    a = _parse(monkeypatch, "--full", "--no-tree", "--cpu-sample", "0")
    assert not a.tree and a.cpu_sample == 0 and a.c4_pods == 20000


def test_steps_beyond_the_queue_are_refused(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--pods", "5", "--steps", "6")
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


class _Sched:
    """Stands in for GenericScheduler: records the (first, count) of every schedule call."""

    def __init__(self, log):
        self.calls = []
        log.append(self)

    def schedule(self, first, count):
        self.calls.append((first, count))
        st = argparse.Namespace(kernel_ms=1.0, kernel_launches=1)
        return np.arange(first, first + count, dtype=np.int32), None, st

    def close(self):
        pass


class _NoDevice:
    barrier = sync = staticmethod(lambda: None)
    allmax = staticmethod(lambda x: x)


@pytest.mark.parametrize("steps,batch,pods", [(20, 50_000, 1_000_000), (9, 5556, 50_000), (3000, 334, 1_000_000),
                                              (6, 2, 10), (10, 512, 5120), (4, 100, 1000), (1, 7, 7)])
def test_timed_queue_runs_exactly_the_steps(steps, batch, pods):
    made = []
    a = argparse.Namespace(warmup=2)
    g, out, el, kms, launches, st, timed, last = bench.timed_queue(a, _NoDevice, lambda: _Sched(made), steps, batch, pods)
    warm, run = made
    assert g is run and len(warm.calls) == 2 and warm.calls[0][0] == 0
    assert len(run.calls) == steps == launches
    assert all(c > 0 for _, c in run.calls)
    assert run.calls[0][0] == 0 and all(f + c == run.calls[i + 1][0] for i, (f, c) in enumerate(run.calls[:-1]))
    covered = min(pods, steps * batch)
    assert timed == covered and np.array_equal(out, np.arange(covered))
    assert last == run.calls[-1][1]
    if covered == steps * batch:
        assert all(c == batch for _, c in run.calls)


def test_dump_outputs_is_float64_bounded_and_repeatable(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 16)
    big = np.arange(1000 * 100, dtype=np.int32).reshape(1000, 100)
    small = np.arange(5, dtype=np.uint64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"placements": big, "counters": small})
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["counters.npy", "placements.npy", "placements_rows.npy"]
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 1 << 16
    rows = got["placements_rows.npy"].astype(int)
    assert len(rows) > 1 and (np.diff(rows) > 0).all()
    assert np.array_equal(got["placements.npy"], big[rows]) and np.array_equal(got["counters.npy"], small)
    for f in files:
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f))
