"""bench.py's N-process contract on the CPU (gloo): ``--gpus N`` without a launcher spawns N ranks
itself, every rank checks WORLD_SIZE == --gpus, and rank 0 prints one JSON line with n_gpus = N.
ANR_BENCH_DRYRUN=1 runs the launch / rendezvous / barrier / max-over-ranks logic with no GPU work."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None):
    env = dict(os.environ, ANR_BENCH_DRYRUN='1', OMP_NUM_THREADS='1')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, capture_output=True,
                          text=True, timeout=240)


def test_gpus_flag_spawns_ranks():
    p = _run(['--gpus', '2', '--steps', '3', '--warmup', '0'])
    assert p.returncode == 0, p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout  # rank 0 only
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['ranks_seen'] == 2 and d['steps'] == 3


def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    return bench.parse()


def test_plain_run_skips_every_extra_leg_and_full_restores_them(monkeypatch):
    legs = ('no_cpu', 'no_exact', 'no_side', 'no_host_render', 'no_torch_baseline')
    a = _parse(['--gpus', '1', '--steps', '7', '--warmup', '2'], monkeypatch)
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert all(getattr(a, k) for k in legs)
    a = _parse(['--full'], monkeypatch)
    assert a.full and not any(getattr(a, k) for k in legs)
    a = _parse(['--full', '--no-side'], monkeypatch)  # each leg can still be switched off under --full
    assert a.no_side and not a.no_cpu


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path):
    import numpy as np
    import torch

    import bench
    rows = bench.DUMP_CAP_BYTES // 16 + 1000  # (rows, 4) float32: just above the per-array cap
    out = {'big': torch.arange(rows * 4, dtype=torch.float32).reshape(1, rows, 4),
           'small': torch.arange(6, dtype=torch.float32).reshape(1, 2, 3),
           'ids': torch.arange(5), 'wide': torch.arange(4, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / 'a'), out)
    bench.dump_outputs(str(tmp_path / 'b'), out)
    got = {f[:-4]: np.load(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')}
    assert sorted(got) == ['big', 'ids', 'small', 'wide']
    assert got['small'].dtype == np.float32 and np.array_equal(got['small'], out['small'].numpy())
    assert got['ids'].dtype == np.float64 and got['wide'].dtype == np.float64
    big = got['big']
    assert big.dtype == np.float32 and big.shape == (bench.DUMP_CAP_BYTES // 16, 4)
    assert big.nbytes <= bench.DUMP_CAP_BYTES
    # whole rows of the source, in ascending row order, the same rows in both runs
    assert np.array_equal(big[:, 1:], big[:, :1] + np.arange(1, 4, dtype=np.float32))
    assert np.all(np.diff(big[:, 0]) > 0)
    assert np.array_equal(big, np.load(tmp_path / 'b' / 'big.npy'))


def test_world_mismatch_fails():
    p = _run(['--gpus', '2'], {'WORLD_SIZE': '1', 'RANK': '0', 'LOCAL_RANK': '0'})
    assert p.returncode != 0
    assert 'WORLD_SIZE=1' in (p.stderr + p.stdout)
