"""CPU: bench.py's command line around the timed steps -- a plain run does only set-up, warm-up, the --steps timed steps,
--dump-outputs and the line; --full adds the other legs -- driven through main() with a stand-in for the device job."""
import json
import sys

import numpy as np
import pytest

LEGS = ("BoxProbe", "profile_kernels", "plain_ntt_rates", "io_leg", "other_configs", "cpu_baseline")


class FakeSet:
    """what dump_outputs needs of a DeviceSet: count and download(first, n)"""

    def __init__(self, count, nl, n, seed):
        self.count, self.shape = count, (count, 2, nl, n)
        self.data = np.random.default_rng(seed).integers(0, 2**59, size=self.shape, dtype=np.uint64)
        self.freed = False

    def download(self, first=0, n=None):
        return self.data[first:first + (self.count - first if n is None else n)].copy()

    def free(self):
        self.freed = True


class FakeCtx:
    def sync(self):
        pass


class FakeJob:
    """Job's surface as main() uses it at one GPU: counts its steps and hands back seeded outputs on keep=True"""
    last = None

    def __init__(self, cfg, rank, world, device, ring_switch_logn=0, allow_replicated=False, local_devices=None):
        self.rows, self.cols, self.log_n, self.L, self.K, self.N = 2048, 1024, 12, 10, 2, 1 << 12
        self.queries, self.key_load_bytes, self.key_load_s = 309, 0, 0.0
        self.ring_switch_logn, self.lane_path, self.group = 0, False, None
        self.ctxs, self.steps, self.kept, self.closed = [FakeCtx()], 0, [], False
        FakeJob.last = self

    def step(self, dist=None, keep=False):
        self.steps += 1
        if not keep:
            return b"\0" * 32
        outs = (FakeSet(self.cols, self.L - 1, self.N, 1), FakeSet(self.cols, self.L - 1, self.N, 2),
                FakeSet(self.queries, 2, self.N, 3), np.arange(64 * 32, dtype=np.uint8).reshape(64, 32) % 251,
                bytes(range(32)))
        self.kept.append(outs)
        return outs

    def close(self):
        self.closed = True


@pytest.fixture
def fake_bench(monkeypatch):
    import torch
    import bench
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (main() sets it by default: restored afterwards)
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(bench, "Job", FakeJob)
    called = []

    def run(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        bench.main()
        return FakeJob.last

    return bench, called, run


def _line(capsys):
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_plain_run_times_the_steps_and_runs_no_other_leg(fake_bench, monkeypatch, capsys):
    bench, _, run = fake_bench

    def refuse(*a, **k):
        raise AssertionError("a plain run must not run this leg")
    for name in LEGS:
        monkeypatch.setattr(bench, name, refuse)
    job = run("--gpus", "1", "--steps", "5", "--warmup", "2")
    assert job.steps == 7 and job.closed and not job.kept
    line = _line(capsys)
    assert line["steps"] == 5 and line["step_ms"]["n"] == 5
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["metric"] == "prove_eval_seconds_16384x4096" and line["unit"] == "s" and line["dtype"] == "u64"
    assert line["higher_is_better"] is False
    assert line["ms_per_step"] == pytest.approx(line["value"] * 1e3, abs=0.1)
    assert "cpu_baseline" not in line and "other_configs" not in line and line["box"] is None and line["roofline"] is None


def test_full_run_still_runs_every_leg(fake_bench, monkeypatch, capsys):
    bench, called, run = fake_bench

    class Probe:
        def __init__(self, device):
            called.append("BoxProbe")

        def start_timed_region(self):
            pass

        def end_timed_region(self):
            return {"identity": {}}
    monkeypatch.setattr(bench, "BoxProbe", Probe)
    monkeypatch.setattr(bench, "profile_kernels", lambda *a: called.append("profile_kernels") or (None, {}, 0, None))
    monkeypatch.setattr(bench, "plain_ntt_rates", lambda *a: called.append("plain_ntt_rates") or {})
    monkeypatch.setattr(bench, "io_leg", lambda *a: called.append("io_leg") or {"marshal_s": 1.0})
    monkeypatch.setattr(bench, "other_configs", lambda *a: called.append("other_configs") or {"2048x1024": {}})
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a: called.append("cpu_baseline") or {"value": 1.0})
    job = run("--gpus", "1", "--steps", "2", "--warmup", "1", "--full")
    assert job.steps == 3
    assert sorted(called) == sorted(LEGS)
    line = _line(capsys)
    assert line["cpu_baseline"] == {"value": 1.0} and line["marshal_s"] == 1.0 and "other_configs" in line


def test_dump_outputs_writes_the_last_timed_step(fake_bench, tmp_path):
    _, _, run = fake_bench
    job = run("--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert job.steps == 4 and len(job.kept) == 1 and all(s.freed for s in job.kept[0][:3])
    names = {p.name for p in (tmp_path / "out").iterdir()}
    assert names == {"mat_r.npy", "mat_z.npy", "queried_cols.npy", "merkle_nodes.npy", "merkle_root.npy"}
    total = 0
    for p in (tmp_path / "out").iterdir():
        a = np.load(p)
        assert a.dtype in (np.float32, np.float64), p.name
        total += a.nbytes
    assert total <= 64 << 20
    root = np.load(tmp_path / "out" / "merkle_root.npy")
    assert np.array_equal(root, np.arange(32, dtype=np.float32))
    # the residues come back exactly from their (low, high) 32-bit halves, at the seeded sample positions
    mat_r = np.load(tmp_path / "out" / "mat_r.npy")
    words = mat_r[..., 0].astype(np.uint64) | (mat_r[..., 1].astype(np.uint64) << np.uint64(32))
    full = job.kept[0][0].data
    assert words.shape[:3] == (32, 2, 9) and words.size <= 1 << 19
    assert np.isin(words[0, 0, 0], full).all()


def test_dump_sample_is_seeded_and_exact():
    from bench_lib.dump import residues_f64, sample
    data = np.random.default_rng(7).integers(0, 2**60, size=(100, 2, 12, 4096), dtype=np.uint64)
    fetch = lambda i: data[i:i + 1]  # noqa: E731
    a, b = sample(100, fetch, seed=5), sample(100, fetch, seed=5)
    assert np.array_equal(a, b) and a.size <= 1 << 19 and a.shape[:3] == (32, 2, 12)
    assert not np.array_equal(a, sample(100, fetch, seed=6))
    small = sample(3, lambda i: data[i:i + 1, :, :1, :8], seed=1)
    assert np.array_equal(small, data[:3, :, :1, :8])  # few and small: everything, in order
    f = residues_f64(data[:2])
    assert f.dtype == np.float64 and f.shape == data[:2].shape + (2,)
    back = f[..., 0].astype(np.uint64) | (f[..., 1].astype(np.uint64) << np.uint64(32))
    assert np.array_equal(back, data[:2])


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", "x"]])
def test_bench_refuses_what_it_cannot_time_or_dump(fake_bench, argv):
    _, _, run = fake_bench
    with pytest.raises(SystemExit) as e:
        run(*argv)
    assert e.value.code == 2
