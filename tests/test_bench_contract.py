"""The driver depends on bench.py's JSON contract (BASELINE.json metric,
one JSON line on stdout from rank 0). Guard it for every bench mode so a
schedule/solver change can't silently break the round-end measurement.

Runs tiny CPU configs (--cpu) of each mode and validates the JSON keys
and value sanity.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_KEYS = {
    'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step',
    'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config',
}


def _run_bench(extra, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--cpu',
           '--steps', '1', '--warmup', '0'] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT,
                         timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    return json.loads(line)


def _check(d):
    assert REQUIRED_KEYS <= set(d), REQUIRED_KEYS - set(d)
    assert d['metric'] == 'visibilities/sec calibrated'
    assert d['value'] > 0 and d['ms_per_step'] > 0
    assert d['higher_is_better'] is True
    assert d['scaling'] == 'weak'
    assert d['data'] == 'synthetic'
    assert isinstance(d['config'], dict) and 'model' in d['config']


def test_bench_default_contract():
    d = _run_bench(['--stations', '8', '--dirs', '2', '--srcs', '2',
                    '--tilesz', '4', '--chan', '2'])
    _check(d)
    assert d['config']['stations'] == 8


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes what the last timed step returned as
    float32/float64 .npy files, identical from run to run (same
    arguments -> same inputs); --full is accepted and keeps the result
    line's contract."""
    import numpy as np
    small = ['--stations', '8', '--dirs', '2', '--srcs', '2',
             '--tilesz', '4', '--chan', '2', '--intervals', '2']
    dumps = []
    for tag, extra in (('a', []), ('b', ['--full'])):
        out = tmp_path / tag
        d = _run_bench(small + ['--dump-outputs', str(out)] + extra)
        _check(d)
        assert d['steps'] == 1
        dumps.append({f: np.load(out / f) for f in sorted(os.listdir(out))})
    a, b = dumps
    assert sorted(a) == ['jones.npy', 'res.npy', 'residuals.npy']
    assert sorted(b) == sorted(a)
    rows = 8 * 7 // 2 * 4 * 2                 # baselines x slots x intervals
    assert a['residuals.npy'].shape == (2, rows, 2, 2, 2)   # [F,B,2,2,re/im]
    assert a['jones.npy'].shape == (2 * 2, 8, 2, 2, 2)      # [Mt,N,2,2,re/im]
    assert a['res.npy'].shape == (2,) and a['res.npy'][1] < a['res.npy'][0]
    total = 0
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), (f, a[f].dtype)
        assert np.isfinite(a[f]).all(), f
        assert np.array_equal(a[f], b[f]), f
        total += a[f].nbytes
    assert total <= 64 * 2**20


def test_bench_dump_outputs_sampling():
    """An array over its share of the dump budget is cut to a fixed,
    seeded sample: same entries every time, complex pairs kept whole."""
    import numpy as np
    import torch
    import bench as bench_mod
    big = torch.arange(3 * 2**21, dtype=torch.float32)
    big = torch.complex(big, -big).reshape(3, -1)
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        bench_mod.dump_outputs(td, {'big': big, 'one': torch.ones(3)})
        s1 = np.load(os.path.join(td, 'big.npy'))
        bench_mod.dump_outputs(td, {'big': big, 'one': torch.ones(3)})
        s2 = np.load(os.path.join(td, 'big.npy'))
        one = np.load(os.path.join(td, 'one.npy'))
    assert s1.dtype == np.float32 and s1.ndim == 2 and s1.shape[1] == 2
    assert s1.nbytes <= bench_mod.DUMP_BUDGET // 2 < big.numel() * 8
    assert np.array_equal(s1, s2)
    assert np.array_equal(s1[:, 0], -s1[:, 1])
    assert np.array_equal(one, np.ones(3, dtype=np.float32))


def test_bench_rtr_contract():
    d = _run_bench(['--stations', '48', '--dirs', '2', '--srcs', '2',
                    '--tilesz', '2', '--chan', '2', '--solver', 'rtr',
                    '--no-consensus'])
    _check(d)


def test_bench_bandpass_contract():
    d = _run_bench(['--mode', 'bandpass', '--stations', '8', '--dirs', '2',
                    '--srcs', '2', '--tilesz', '2', '--chan', '16',
                    '--nsolbw', '4'])
    _check(d)


def test_bench_two_rank_launch():
    """Launch bench.py exactly the way the driver's scaling harness does
    (torch.distributed.run, one process per 'GPU', 127.0.0.1 rendezvous)
    with 2 CPU/gloo ranks: rank 0 must print the JSON contract line with
    the whole-job aggregate value."""
    env = dict(os.environ)
    env['SAGECAL_BENCH_BACKEND'] = 'gloo'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29547', os.path.join(ROOT, 'bench.py'),
           '--gpus', '2', '--cpu', '--steps', '1', '--warmup', '0',
           '--stations', '8', '--dirs', '2', '--srcs', '2',
           '--tilesz', '4', '--chan', '2']
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT,
                         env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.strip().splitlines()
            if l.startswith('{')][-1]
    d = json.loads(line)
    _check(d)
    assert d['config']['parallelism'].endswith('2')


def test_bench_eight_rank_launch():
    """The driver's 8-GPU scale run shape, on CPU/gloo: 8 ranks, one
    band each, fused consensus all-reduce; rank 0 prints the aggregate
    JSON line."""
    env = dict(os.environ)
    env['SAGECAL_BENCH_BACKEND'] = 'gloo'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           '--nproc-per-node', '8', '--master-addr', '127.0.0.1',
           '--master-port', '29549', os.path.join(ROOT, 'bench.py'),
           '--gpus', '8', '--cpu', '--steps', '1', '--warmup', '0',
           '--stations', '8', '--dirs', '2', '--srcs', '2',
           '--tilesz', '2', '--chan', '2']
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT,
                         env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.strip().splitlines()
            if l.startswith('{')][-1]
    d = json.loads(line)
    _check(d)
    assert d['config']['parallelism'].endswith('8')


def test_bench_interval_clamp(monkeypatch):
    """--intervals is clamped to the coherency residency budget for
    very large arrays (guard against OOM at naive 512+/16 settings)."""
    import bench as bench_mod
    import sagecal_amd.msdata as md

    class A:
        pass
    a = A()
    a.__dict__.update(stations=2048, dirs=20, srcs=5, tilesz=60,
                      chan=8, freq0=150e6, bandwidth=180e3,
                      intervals=16, shapelet_dirs=0)
    seen = {}

    def fake_init(self, **kw):
        seen['tilesz'] = kw.get('tilesz')
        raise SystemExit
    monkeypatch.setattr(md.SyntheticMS, '__init__', fake_init)
    try:
        bench_mod.build_problem(a, 'cpu', None)
    except SystemExit:
        pass
    assert a.intervals == 1                  # clamped from 16
    assert seen['tilesz'] == 60              # tilesz * clamped intervals
